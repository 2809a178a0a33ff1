"""The signal catalogue (tests/signals.py) still has the structure each signal exists
for, asserted from the oracle alone (no GPU): a later edit of a builder, of the chain
settings or of the oracle cannot quietly turn a structured case back into a
stationary one.  These are conditions on the inputs of tests/test_gpu_signals.py,
not measurements of the device."""
import functools

import numpy as np
import pytest

import signals as S

PARAMS = {"hot": S.P_HOT, "full": S.P_FULL}


@functools.lru_cache(maxsize=None)
def _structure(name, channels=2, params="hot"):
    build = S.chunk_seam if name == "chunk_seam" else S.CATALOGUE[name]
    return S.structure(build(channels=channels), S.RATE, PARAMS[params])


def _bands(st):
    return [b for chunk in st["chunks"] for b in chunk]


def test_builders_are_deterministic_int16():
    for name, build in S.CATALOGUE.items():
        for ch in (1, 2):
            a, b = build(channels=ch), build(channels=ch)
            assert a.dtype == np.int16 and a.shape == ((132300,) if ch == 1 else (132300, 2)), name
            assert np.array_equal(a, b), name
        assert build(seconds=0.5, rate=48000).shape == (24000, 2), name
    assert S.chunk_seam().shape == (31 * 44100, 2)


@pytest.mark.parametrize("params", ["hot", "full"])
@pytest.mark.parametrize("channels", [2, 1])
def test_bursts_are_sparse(channels, params):
    for b in _bands(_structure("bursts", channels, params)):
        assert b["quiet"] >= 0.5 * b["tiles"], b["quiet"]
        assert b["full"] >= 0.1 * b["tiles"], b["full"]


@pytest.mark.parametrize("params", ["hot", "full"])
def test_square_is_partial_and_full_scale(params):
    bands = _bands(_structure("square_fs", 2, params))
    assert max(b["partial"] / b["tiles"] for b in bands) >= 0.5
    assert max(b["max_rms"] for b in bands) >= 30000


def test_step_down_is_relatively_gated():
    L = _structure("step_down")["loudness"]
    assert 2 * L["rel_gated"] >= len(L["blocks"]), (L["rel_gated"], len(L["blocks"]))
    assert max(b["quiet"] for b in _bands(_structure("step_down"))) >= 400  # a long release over quiet tiles


@pytest.mark.parametrize("channels", [2, 1])
def test_fade_in_cut_meets_both_gates(channels):
    st = _structure("fade_in_cut", channels)
    L = st["loudness"]
    assert L["abs_gated"] >= 3 and L["rel_gated"] >= 3, (L["abs_gated"], L["rel_gated"])
    assert L["abs_gated"] + L["rel_gated"] < len(L["blocks"])
    over = L["blocks"][L["blocks"] > L["gamma_r"]] - L["gamma_r"]
    assert 0.1 <= over.min() <= 0.9, over.min()  # one block passes the relative gate by under 1 LU
    for b in _bands(st):  # the first active tile of every band lies late in the chunk
        first = int(np.argmax(b["M"] > 0.0)) // st["tile"]
        assert b["active"] > 0 and first >= 256, first


def test_clicks_leave_bands_without_active_frames():
    act = [b["active"] for b in _bands(_structure("clicks"))]
    assert min(act) == 0 and max(act) > 0, act
    assert _structure("clicks")["loudness"]["loudness"] < -30.0  # the gain drives the limiter


def test_sub_gate_is_not_silent_but_gated():
    pcm = S.sub_gate()
    assert pcm.any()
    st = _structure("sub_gate")
    assert st["loudness"]["loudness"] == -np.inf
    assert st["loudness"]["abs_gated"] == len(st["loudness"]["blocks"])
    assert not S.oracle.master(pcm, S.RATE, S.P_HOT).any()  # inf gain -> NaN -> 0, as silence_1s.npz


def test_chunk_seam_straddles():
    """Both chunks have active frames next to the seam in every band."""
    st = _structure("chunk_seam")
    assert len(st["chunks"]) == 2
    for b0, b1 in zip(*st["chunks"]):
        assert (b0["M"][-1000:] > 0.0).any() and (b1["M"][:1000] > 0.0).any()


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [44100, 48000])
def test_const_fs_reads_the_last_row(rate, channels):
    x = S.const_fs(channels=channels)
    thr, ratio, at, rel = S.band_settings()[0]
    b = S.band_structure(x, rate, thr, ratio, at, rel, 125)
    assert b["max_rms"] == 32768
    y, att = S.oracle.compress_band(x, rate, thr, ratio, at, rel, return_att=True)
    assert abs(att[-1] - 125.0 / 6.0) < 1e-9 and y.flat[-1] == -2978, (att[-1], y.flat[-1])


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [44100, 48000])
def test_staircase_sits_binades_above_m(rate, channels):
    bands = S.staircase_bands(channels)
    assert not bands[2].any()
    for x, (thr, ratio, at, rel) in zip(bands[:2], S.band_settings()):
        r0 = S.band_r0(thr, ratio)
        b = S.band_structure(x, rate, thr, ratio, at, rel, 125)
        assert b["binades"] >= 9, b["binades"]
        rms = S.window_rms(x, int(at * (rate / 1000.0)))
        assert {r0 - 1, r0, r0 + 1, r0 + 2, 20000, 0} <= set(np.unique(rms).tolist())  # constant v: rms == |v|
    assert S.band_r0(-20.0, 3.0) == 3277


GPU_LOUDNESS_CASES = [(n, 2, "hot") for n in S.CATALOGUE] + [("bursts", 1, "hot"), ("fade_in_cut", 1, "hot"),
                                                             ("chunk_seam", 2, "hot")]


@pytest.mark.parametrize("name,channels,params", GPU_LOUDNESS_CASES)
def test_no_block_near_a_gate(name, channels, params):
    """Every signal whose loudness the GPU tests measure: no block within 0.01 LU of
    -70 LUFS or of the relative threshold, so a last-bit difference in a block energy
    cannot flip a gate decision; and the restated gating gives the oracle's loudness."""
    L = _structure(name, channels, params)["loudness"]
    assert S.gate_margin(L) >= 0.01, S.gate_margin(L)
    z = 10.0 ** ((L["blocks"] + 0.691) / 10.0)
    keep = (L["blocks"] > L["gamma_r"]) & (L["blocks"] > -70.0)
    if keep.any():
        assert abs(-0.691 + 10.0 * np.log10(z[keep].mean()) - L["loudness"]) < 1e-9
    else:
        assert L["loudness"] == -np.inf


def test_structure_counts_what_the_oracle_attenuates():
    """structure()'s active frames against the oracle's own trajectory: a frame with
    rms >= r0 has M > 0, so the attenuation after it is nonzero."""
    pcm = S.bursts()
    thr, rat = S.oracle.multiband_params(S.P_HOT)
    x = S.oracle.stereo_width(S.oracle.equalize(S.oracle.saturation(S.oracle.pcm_to_float(pcm), 30), S.RATE, S.P_HOT),
                              1.3)
    st = _structure("bursts")
    for band, b, t, r, (at, rel) in zip(S.oracle.band_split(S.oracle.quantize(x), S.RATE), st["chunks"][0], thr, rat,
                                        S.oracle.BAND_TIMES):
        _, att = S.oracle.compress_band(band, S.RATE, t, r, at, rel, return_att=True)
        assert b["active"] == int((b["M"] > 0.0).sum()) > 0
        assert np.all(att[b["M"] > 0.0] > 0.0)
