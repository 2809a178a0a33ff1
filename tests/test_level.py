"""Delivery to an R 128 loudness target on CPU: the library's host restatement (mm_level_host)
against forty lines of numpy written from the definition in include/mastering.h (mm_level)
on top of the ceiling's and the R 128 report's own numpy definitions, the properties the
definition promises, the struct layouts and the Python plumbing that needs no GPU.  Samples
and integer statistics are compared for equality; the loudness figures, which both sides
compute from the same samples with sums in another order, within 1e-6 LU."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_ceiling import GUARD, ONE, q28, ref_ceiling
from test_meter import ref_meter
from test_r128 import ref_hops, ref_r128, stepped_noise

RATE = 44100
PASSES, TOL, SMIN = 5, 0.05, 0.25
INTS = ("frames", "channels", "rate", "target_clu", "ceiling_q28", "window", "status", "passes", "gain_q16",
        "min_gain_q16", "clipped", "limited_frames")
STATUS = {"off": 0, "reached": 1, "capped": 2, "saturated": 3, "passes": 4, "unmeasurable": 5}


# ------------------------------------------------------------ the definition, in numpy
def ref_gain(x, g):
    """gain(x, g): (samples, clipped)."""
    y = (np.asarray(x).astype(np.int64) * g + (1 << 15)) >> 16
    d = np.clip(y, -32768, 32767)
    return d.astype(np.int16), int((d != y).sum())


def q(G):
    return int(min(max(math.floor(G * 65536.0 + 0.5), 1 << 8), 1 << 21))


def integrated(x, rate):
    return float(ref_r128(ref_hops(x, rate), rate)["integrated"])


def ref_pass(pcm, g, C, W):
    """Step 3 for one gain: (y_k, the gain after its cap, capped, clipped, the limiting ceil call's stats)."""
    capped, lim = False, None
    if not C:
        g_peak = min((32767 << 16) // int(np.abs(pcm.astype(np.int64)).max()), 1 << 21)
        g, capped = (g_peak, True) if g > g_peak else (g, False)
        y, clipped = ref_gain(pcm, g)
    elif g <= ONE:
        y, clipped = ref_gain(pcm, g)
        y, lim = ref_ceiling(y, C, W)
    else:
        g_cap = ((C - GUARD) << 16) >> 24
        g, capped = (g_cap, True) if g > g_cap else (g, False)
        u, lim = ref_ceiling(pcm, ((C - GUARD) << 16) // g, W)
        y, clipped = ref_gain(u, g)
        y, last = ref_ceiling(y, C, W)
        lim = dict(lim, final_touched=last["tp_in_q28"] > C, tp_out_q28=last["tp_out_q28"])
    return y, g, capped, clipped, lim


def ref_level(pcm, rate, T, C, W, gains=None):
    """The definition of mm_level: (delivered samples, stats).  `gains`: replay exactly these
    pass gains without deciding anything (the last pass is delivered)."""
    pcm = np.asarray(pcm)
    st = dict(status="unmeasurable", passes=0, gain_q16=ONE, pass_gain_q16=[], pass_lufs=[], loudness=math.nan,
              source_lufs=integrated(pcm, rate), clipped=0, min_gain_q16=ONE, limited_frames=0, margins=[], slopes=[])
    if not math.isfinite(st["source_lufs"]):
        if C:
            y, lim = ref_ceiling(pcm, C, W)
            st.update(min_gain_q16=lim["min_gain_q16"], limited_frames=lim["limited_frames"])
        return (y if C else pcm.copy()), st
    g, st["status"] = q(10.0 ** ((T - st["source_lufs"]) / 20.0)), None
    for k in range(PASSES if gains is None else len(gains)):
        y, g, capped, st["clipped"], lim = ref_pass(pcm, g if gains is None else gains[k], C, W)
        st["pass_gain_q16"].append(g)
        st["pass_lufs"].append(integrated(y, rate))
        st.update(passes=k + 1, gain_q16=g, loudness=st["pass_lufs"][k], lim=lim)
        if lim:
            st.update(min_gain_q16=lim["min_gain_q16"], limited_frames=lim["limited_frames"])
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
    return y, st


# ------------------------------------------------------------ the library
def host_level(pcm, rate, T, C, W, ceiling=None):
    """(delivered samples, mm_level) of mm_level_host."""
    from mastering_amd import design, engine, native
    x = np.array(pcm, np.int16, order="C")  # a copy: the call works in place
    m = native.MMLevel()
    rc = native.load().mm_level_host(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), x.shape[0],
                                     1 if x.ndim == 1 else x.shape[1], rate, engine.kweight_sos(rate),
                                     design.level_clu(T), C, W, ctypes.byref(m),
                                     ctypes.byref(ceiling) if ceiling is not None else None)
    assert rc == 0
    return x, m


def level_ints(m):
    d = {f: int(getattr(m, f)) for f in INTS}
    d["pass_gain_q16"] = [int(v) for v in m.pass_gain_q16]
    return d


def pink(seconds, channels, level, track, rate=RATE):
    from mastering_amd.synth import pink_noise_pcm16
    return pink_noise_pcm16(int(seconds * rate), rate, channels, track=track, level_dbfs=level)


def case_inputs():
    """name -> (pcm, rate, target, C, W, status, passes): the outcomes are those of the rule's
    numpy prototype on these signals (asserted on ref_level itself in `refs`)."""
    C = q28(-1.0)
    return {
        "down": (pink(3, 2, -12.0, 1), RATE, -20.0, C, 220, "reached", 1),
        "up-idle": (pink(3, 2, -18.0, 2), RATE, -12.0, C, 220, "reached", 1),
        "stepped": (stepped_noise(4 * RATE, RATE, 2), RATE, -13.0, C, 220, "reached", 2),
        "mono-boost": (pink(3, 1, -18.0, 3), RATE, -11.0, C, 220, "reached", 3),
        "saturated": (pink(3, 2, -18.0, 2), RATE, -7.0, C, 220, "saturated", 2),
        "capped": (pink(3, 2, -60.0, 4), RATE, -10.0, C, 220, "capped", 1),
        "no-ceiling": (pink(3, 2, -12.0, 1), RATE, -8.0, 0, 220, "capped", 1),
        "window-1": (pink(3, 1, -18.0, 3), RATE, -11.0, C, 1, "reached", None),
    }


@pytest.fixture(scope="module")
def cases():
    return case_inputs()


@pytest.fixture(scope="module")
def refs(cases):
    """ref_level of every case (shared, read-only), with the margins that keep every decision
    of the rule stable against the 1e-6 LU by which two correct meters may differ."""
    out = {}
    for name, (pcm, rate, T, C, W, status, passes) in cases.items():
        y, st = ref_level(pcm, rate, T, C, W)
        print(name, st["status"], st["passes"], st["pass_gain_q16"], [round(v, 4) for v in st["pass_lufs"]],
              "margins", st["margins"], st["slopes"])
        assert st["status"] == status and (passes is None or st["passes"] == passes), name
        assert min(st["margins"]) >= 1e-3, name
        assert min(st["slopes"], default=1.0) >= 0.01, name
        out[name] = (y, st)
    return out


NAMES = ["down", "up-idle", "stepped", "mono-boost", "saturated", "capped", "no-ceiling", "window-1"]


# ------------------------------------------------------------ tests
@pytest.mark.parametrize("name", NAMES)
def test_host_restatement(cases, refs, name):
    pcm, rate, T, C, W, _, _ = cases[name]
    want, st = refs[name]
    ce = None
    if C:
        from mastering_amd import native
        ce = native.MMCeiling()
    got, m = host_level(pcm, rate, T, C, W, ce)
    assert np.array_equal(got, want)
    assert m.status == STATUS[st["status"]] and m.passes == st["passes"]
    for k in range(m.passes):
        assert abs(m.pass_gain_q16[k] - st["pass_gain_q16"][k]) <= 1, k
    assert (m.frames, m.channels, m.rate, m.target_clu, m.ceiling_q28, m.window) == \
        (len(pcm), pcm.reshape(len(pcm), -1).shape[1], rate, round(100 * T), C, W)
    # the reference again with the library's recorded gains: the same bytes and figures
    gains = [int(m.pass_gain_q16[k]) for k in range(m.passes)]
    again, rst = ref_level(pcm, rate, T, C, W, gains)
    assert np.array_equal(got, again)
    for k in range(m.passes):
        assert abs(m.pass_lufs[k] - rst["pass_lufs"][k]) <= 1e-6, k
    assert all(math.isnan(m.pass_lufs[k]) and m.pass_gain_q16[k] == 0 for k in range(m.passes, PASSES))
    assert abs(m.source_lufs - rst["source_lufs"]) <= 1e-6 and abs(m.loudness - rst["loudness"]) <= 1e-6
    assert m.gain_q16 == gains[-1] and m.loudness == m.pass_lufs[m.passes - 1]
    assert (m.clipped, m.min_gain_q16, m.limited_frames) == (rst["clipped"], rst["min_gain_q16"], rst["limited_frames"])
    if st["status"] == "reached":
        assert abs(m.loudness - T) <= TOL
    if C:  # the delivered true peak is mm_ceiling's own guarantee, and the struct is the final call's
        tp = max(ref_meter(got)["true_peak_q28"])
        assert tp <= C and ce.tp_out_q28 == tp and ce.ceiling_q28 == C and ce.frames == len(pcm)
        if rst["lim"] and "final_touched" in rst["lim"]:
            assert not rst["lim"]["final_touched"] and ce.limited_frames == 0  # the boost branch's proof
    else:
        assert m.clipped == 0 and np.abs(got.astype(np.int64)).max() <= 32767


def test_the_cases_take_every_branch(refs):
    assert refs["capped"][1]["gain_q16"] == 934511 == ((q28(-1.0) - GUARD) << 16) >> 24
    assert refs["stepped"][1]["gain_q16"] <= ONE and refs["stepped"][1]["limited_frames"] > 0
    assert refs["up-idle"][1]["gain_q16"] > ONE and refs["up-idle"][1]["limited_frames"] == 0
    assert refs["mono-boost"][1]["gain_q16"] > ONE and refs["mono-boost"][1]["limited_frames"] > 0
    assert refs["down"][1]["gain_q16"] < ONE
    assert refs["saturated"][1]["loudness"] < -7.0 - TOL
    assert refs["no-ceiling"][1]["loudness"] < -8.0 - TOL


def test_one_is_the_identity_and_minus_one_by_half_is_zero():
    x = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    y, clipped = ref_gain(x, ONE)
    assert np.array_equal(y, x) and clipped == 0
    assert ref_gain(np.array([-1], np.int16), 1 << 15)[0][0] == 0  # (-2^15 + 2^15) >> 16
    assert ref_gain(np.array([1], np.int16), 1 << 15)[0][0] == 1   # ties go up: the shift is a floor
    y, clipped = ref_gain(np.array([-32768, 32767, 1], np.int16), 1 << 21)
    assert y.tolist() == [-32768, 32767, 32] and clipped == 2
    # the library's gain is this one: a level without a ceiling delivers gain(source, its recorded g)
    pcm = pink(3, 2, -18.0, 5)
    got, m = host_level(pcm, RATE, round(integrated(pcm, RATE), 2), 0, 220)
    assert m.status == STATUS["reached"] and m.passes == 1 and abs(m.gain_q16 - ONE) <= 40  # (0.005 LU: 38 steps)
    assert np.array_equal(got, ref_gain(pcm, int(m.gain_q16))[0])


@pytest.mark.parametrize("what", ["short", "silence"])
@pytest.mark.parametrize("C", [0, q28(-1.0)], ids=["no-ceiling", "ceiling"])
def test_unmeasurable(what, C):
    """17 000 frames are fewer than 4 hops (NaN); silence has no block over the gate (-inf):
    the ceiling alone acts, and the true peak still ends under it."""
    from mastering_amd import native
    pcm = pink(1, 2, -3.0, 6)[:17000] if what == "short" else np.zeros((RATE, 2), np.int16)
    want, st = ref_level(pcm, RATE, -14.0, C, 220)
    ce = native.MMCeiling()
    got, m = host_level(pcm, RATE, -14.0, C, 220, ce)
    assert st["status"] == "unmeasurable" and m.status == STATUS["unmeasurable"] and m.passes == 0
    assert m.gain_q16 == ONE and math.isnan(m.loudness) and np.array_equal(got, want)
    assert math.isnan(m.source_lufs) if what == "short" else m.source_lufs == -math.inf
    assert (m.min_gain_q16, m.limited_frames) == (st["min_gain_q16"], st["limited_frames"])
    if C:
        assert max(ref_meter(got)["true_peak_q28"]) <= C
        assert (what == "short") == (m.limited_frames > 0)
    else:
        assert np.array_equal(got, pcm)


def test_host_refusals():
    from mastering_amd import engine, native
    lib = native.load()
    x = np.zeros((100, 2), np.int16)
    p, m, sos = x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), native.MMLevel(), engine.kweight_sos(RATE)
    C = q28(-1.0)
    ok = lambda *a: lib.mm_level_host(*a, ctypes.byref(m), None)  # noqa: E731
    assert ok(p, 100, 2, RATE, sos, -1400, C, 220) == 0
    assert ok(p, 100, 2, RATE, sos, -4000, 0, 0) == 0 and ok(p, 100, 2, RATE, sos, -500, 0, 0) == 0
    for clu in (0, -4001, -499, 1400):
        assert ok(p, 100, 2, RATE, sos, clu, C, 220) == native.MM_ERR_ARG
    assert ok(p, 100, 3, RATE, sos, -1400, C, 220) == native.MM_ERR_ARG
    assert ok(p, 100, 2, 1999, sos, -1400, C, 220) == native.MM_ERR_ARG
    assert ok(p, 100, 2, RATE, None, -1400, C, 220) == native.MM_ERR_ARG
    assert ok(p, 100, 2, RATE, sos, -1400, 2 ** 24 - 1, 220) == native.MM_ERR_ARG
    assert ok(p, 100, 2, RATE, sos, -1400, C, 0) == native.MM_ERR_ARG
    assert ok(p, 100, 2, RATE, sos, -1400, C, 1025) == native.MM_ERR_ARG
    assert ok(None, 100, 2, RATE, sos, -1400, C, 220) == native.MM_ERR_ARG
    assert lib.mm_level_host(p, 100, 2, RATE, sos, -1400, C, 220, None, None) == native.MM_ERR_ARG
    assert lib.mm_level_span() % 8 == 0 and lib.mm_level_span() >= 8


def test_level_layouts_match_c(tmp_path):
    from mastering_amd import native
    fields = {"mm_level": native.MMLevel, "mm_delivery": native.MMDelivery}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){"]
    for st, cls in fields.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("abi %d\\n", MM_ABI_VERSION);')
    lines.append('printf("status %d\\n", MM_LEVEL_OFF + 10 * (MM_LEVEL_REACHED + 10 * (MM_LEVEL_CAPPED + 10 * ('
                 'MM_LEVEL_SATURATED + 10 * (MM_LEVEL_PASSES_SPENT + 10 * MM_LEVEL_UNMEASURABLE)))));')
    lines.append('printf("passes %d\\n", MM_LEVEL_PASSES);')
    lines.append("return 0;}")
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for st, cls in fields.items():
        assert int(got[st]) == ctypes.sizeof(cls), st
        for f, _ in cls._fields_:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert int(got["mm_delivery"]) == 32 and int(got["mm_delivery.level_clu"]) == 20  # the former pad
    assert int(got["abi"]) == native.ABI_VERSION == native.load().mm_version() == 5
    assert int(got["status"]) == 543210 and native.LEVEL_STATUS == tuple(STATUS)
    assert int(got["passes"]) == native.LEVEL_PASSES == PASSES


def test_design_level_clu():
    from mastering_amd import design
    assert design.level_clu(-14) == -1400 and design.level_clu(-14.004) == -1400 and design.level_clu(-23.5) == -2350
    assert design.level_clu(-40) == -4000 and design.level_clu(-5.0) == -500
    for bad in (-40.01, -4.99, 0, 14, float("nan")):
        with pytest.raises(ValueError):
            design.level_clu(bad)


def test_job_plans_the_level():
    from mastering_amd import design, engine
    p = {"multiband": True, "lufs": -14.0}
    plain = engine.Job(96000, 96000, 2, p, report=True, ceiling_dbtp=-1.0, r128=True)
    assert plain.delivery is None and plain.deliver_lufs is None
    job = engine.Job(96000, 96000, 2, p, report=True, ceiling_dbtp=-1.0, r128=True, deliver_lufs=-14.0)
    d = job.delivery
    assert not d.rs and job.resampler is None and job.output_rate is None and job.frames_out == job.frames_proc
    assert (job.job.meter_on, job.job.ceiling_q28) == (0, 0) and job.job.lufs_on == 1 and job.deliver_lufs == -14.0
    assert (d.level_clu, d.meter_on, d.ceiling_q28, d.window) == (-1400, 3, design.ceiling_q28(-1.0), design.ceiling_window(96000))
    loud = d.loud.contents
    assert (loud.frames_proc, loud.rate, loud.channels, loud.kweight.nsec) == (job.frames_proc, 96000, 2, 2)
    assert tuple(loud.kweight.sos[0]) == tuple(map(float, design.kweight_sections(96000)[0]))
    # everything before the moved fields is the plain job's
    assert bytes(job.job)[:64] == bytes(plain.job)[:64]
    bare = engine.Job(96000, 96000, 1, {}, deliver_lufs=-23.0).delivery
    assert (bare.level_clu, bare.meter_on, bare.ceiling_q28) == (-2300, 0, 0) and bare.loud.contents.kweight.nsec == 2
    # with another rate: the converter, and the sections of the output's rate
    job = engine.Job(96000, 96000, 2, p, ceiling_dbtp=-1.0, output_rate=44100, deliver_lufs=-16.0)
    d = job.delivery
    assert d.rs.contents.rate_out == 44100 and d.level_clu == -1600 and d.window == design.ceiling_window(44100)
    assert d.loud.contents.rate == 44100 and d.loud.contents.frames_proc == job.frames_out
    assert tuple(d.loud.contents.kweight.sos[1]) == tuple(map(float, design.kweight_sections(44100)[1]))
    assert engine.Job(96000, 96000, 2, p, output_rate=44100).delivery.level_clu == 0
    for bad in (-41.0, -4.0, 0.0):
        with pytest.raises(ValueError):
            engine.Job(96000, 96000, 2, p, deliver_lufs=bad)


def test_paths_without_the_whole_chain_refuse_the_key():
    from mastering_amd import distributed, engine, legacy
    with pytest.raises(ValueError, match="deliver_lufs"):
        engine.Job(44100, 44100, 2, {"lufs": -14.0}, seg_bounds=[0, 4410, 44100], check_length=False, deliver_lufs=-14.0)
    with pytest.raises(ValueError, match="deliver_lufs"):
        engine.Job(44100, 44100, 2, {}, single_chunk=True, deliver_lufs=-14.0)
    with pytest.raises(ValueError, match="deliver_lufs"):
        distributed.master_time_sharded(None, None, {"deliver_lufs": -14.0}, None, None, None)
    with pytest.raises(ValueError, match="deliver_lufs"):
        legacy.master_pcm(np.zeros((100, 2), np.int16), 44100, {"deliver_lufs": -14.0})
    with pytest.raises(ValueError, match="deliver_lufs"):
        legacy.process("no-such-file.wav", "out.wav", {"deliver_lufs": -14.0})
    jobs = [engine.Job(44100, 44100, 2, {}, deliver_lufs=-14.0)]
    with pytest.raises(ValueError, match="deliver_lufs"):
        engine.master_batch(None, jobs, [0], [0])


def test_level_dict():
    from mastering_amd import engine, native
    m = native.MMLevel()
    m.frames, m.channels, m.rate, m.target_clu, m.ceiling_q28, m.window = 1000, 2, 48000, -1400, 2 ** 27, 240
    m.status, m.passes, m.gain_q16, m.min_gain_q16, m.clipped, m.limited_frames = 3, 2, 2 ** 17, 2 ** 15, 4, 9
    m.pass_gain_q16[0], m.pass_gain_q16[1], m.pass_lufs[0], m.pass_lufs[1] = 2 ** 18, 2 ** 17, -13.0, -14.5
    m.pass_lufs[2] = math.nan
    m.source_lufs, m.loudness = -20.0, -14.5
    d = engine.level_dict(m)
    assert d["status"] == "saturated" and d["target_lufs"] == -14.0 and d["passes"] == 2
    assert d["pass_gain_q16"] == [2 ** 18, 2 ** 17] and d["pass_lufs"] == [-13.0, -14.5]
    assert d["pass_gain_db"] == [20 * math.log10(4.0), 20 * math.log10(2.0)] and d["gain_db"] == 20 * math.log10(2.0)
    assert d["max_reduction_db"] == -20 * math.log10(0.5) and d["clipped"] == 4 and d["limited_frames"] == 9
    assert d["source_lufs"] == -20.0 and d["loudness"] == -14.5 and d["ceiling_q28"] == 2 ** 27 and d["window"] == 240
    m.status, m.passes, m.source_lufs, m.loudness = 5, 0, -math.inf, math.nan
    d = engine.level_dict(m)
    assert d["status"] == "unmeasurable" and d["source_lufs"] is None and d["loudness"] is None and d["pass_lufs"] == []
    assert json.dumps(d)  # strict JSON as it stands


def test_master_pcm_pops_the_key_before_planning(monkeypatch):
    from mastering_amd import engine, gui_compat
    seen = {}

    class Stop(Exception):
        pass

    def job(*a, **kw):
        seen.update(kw, params=a[3])
        raise Stop

    monkeypatch.setattr(engine, "Job", job)
    with pytest.raises(Stop):
        engine.master_pcm(np.zeros((10, 2), np.int16), 44100, {"deliver_lufs": -14.0, "width": 1.2})
    assert seen["deliver_lufs"] == -14.0 and seen["params"] == {"width": 1.2}
    seen.clear()
    with pytest.raises(Stop):
        engine.master_pcm(np.zeros((10, 2), np.int16), 44100, {"width": 1.2})
    assert seen["deliver_lufs"] is None
    assert gui_compat.chain_settings({"deliver_lufs": -14.0, "input_file": "a"}) == {"deliver_lufs": -14.0}


def test_gui_and_worker_pass_the_level_through(tmp_path, monkeypatch):
    from mastering_amd import engine, gui_compat
    from mastering_amd.worker import process_audio_from_gcs
    level = {"target_lufs": -14.0, "status": "reached", "loudness": -14.02, "gain_db": 3.41, "passes": 2}
    seen = []

    def process(src, dst, params, device=0, verbose=False):
        seen.append(dict(params))
        with open(dst, "wb") as f:
            f.write(b"RIFF")
        return {"loudness": -20.0, "level": dict(level)} if "deliver_lufs" in params else {"loudness": -20.0}

    monkeypatch.setattr(engine, "process", process)
    said = []
    s = {"input_file": str(tmp_path / "a.wav"), "output_file": str(tmp_path / "b.wav"), "lufs": -14.0}
    gui_compat.process_audio(dict(s, deliver_lufs=-14.0), said.append)
    assert seen[-1]["deliver_lufs"] == -14.0
    assert said[-2] == "Level -14.00 LUFS: reached, delivered -14.02 LUFS with +3.41 dB in 2 passes"
    assert gui_compat.level_line(dict(level, status="unmeasurable", loudness=None, passes=0)) == \
        "Level -14.00 LUFS: unmeasurable, nothing to measure"
    said.clear()
    gui_compat.process_audio(s, said.append)
    assert not any(m.startswith("Level") for m in said)
    (tmp_path / "b").mkdir()
    (tmp_path / "b" / "x.wav").write_bytes(b"")
    out = tmp_path / "b" / "processed" / "mastered_x.wav"
    process_audio_from_gcs("gs://b/x.wav", {"lufs": -14.0}, root=str(tmp_path))
    assert out.exists() and not os.path.exists(str(out) + ".level.json")
    process_audio_from_gcs("gs://b/x.wav", {"lufs": -14.0, "deliver_lufs": -14.0}, root=str(tmp_path))
    assert seen[-1]["deliver_lufs"] == -14.0
    assert json.loads(open(str(out) + ".level.json").read()) == level
    assert os.path.exists(str(out) + ".complete") and not list((tmp_path / "b" / "processed").glob("*.part"))
