"""The host restatements of the level (mm_level_host, mm_album_level_host) against what they gave
before they shared one loop: tests/golden/level_host_parent.json, recorded by
tests/golden/make_level_host_parent.py on the seeded inputs that tests/test_level.py,
tests/test_album.py, tests/test_gpu_level.py, tests/test_gpu_album.py and
tests/test_gpu_batch_level.py build.  Every delivered track by its SHA-256, every field of every
struct for equality, the doubles as hex floats.  The host restatements are the oracle of the GPU
tests, and this file is the oracle of the host restatements."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_ceiling import q28

PATH = os.path.join(GOLDEN, "level_host_parent.json")
RATE = 44100


@functools.lru_cache(maxsize=None)
def level_cases():
    """name -> (pcm, rate, target, C, W) of every single-track input of the level's tests."""
    import test_level
    from mastering_amd import native
    from mastering_amd.synth import pink_noise_pcm16
    C = q28(-1.0)
    out = {name: v[:5] for name, v in test_level.case_inputs().items()}
    short, silence = test_level.pink(1, 2, -3.0, 6)[:17000], np.zeros((RATE, 2), np.int16)
    for c, tag in ((0, "no-ceiling"), (C, "ceiling")):
        out[f"short-{tag}"] = (short, RATE, -14.0, c, 220)
        out[f"silence-{tag}"] = (silence, RATE, -14.0, c, 220)
    out["empty"] = (np.zeros((0, 2), np.int16), RATE, -14.0, C, 220)
    out["mono-48k"] = (test_level.pink(3, 1, -18.0, 7, rate=48000), 48000, -14.0, C, 240)
    mono_short = pink_noise_pcm16(17000, RATE, 1, track=5, level_dbfs=-12.0)
    for W in (220, 1):
        out[f"mono-short-w{W}"] = (mono_short, RATE, -14.0, C, W)
    span = native.load().mm_level_span()
    for i, (n, T) in enumerate(zip((5, span + 3, 3 * 8000), (-14.0, -15.0, -13.0))):
        out[f"views-{i}"] = (pink_noise_pcm16(n, 8000, 1, track=60 + i, level_dbfs=-18.0), 8000, T, C, 40)
    return out


@functools.lru_cache(maxsize=None)
def album_cases():
    """name -> (tracks, rate, target, C, W) of every album of the level's tests."""
    import test_album
    C = q28(-1.0)
    cases = test_album.case_inputs()
    out = {name: (v[0], RATE) + tuple(v[1:4]) for name, v in cases.items()}
    for name, pcm, T, c in (("one-cut", cases["cut"][0][0], -15.0, C), ("one-boost", cases["boost-2"][0][0], -12.0, C),
                            ("one-no-ceiling", cases["boost-2"][0][0], -8.0, 0), ("one-short", cases["cut"][0][3], -14.0, C)):
        out[name] = ([pcm], RATE, T, c, 220)
    out["fates"] = test_album.album_fates()
    return out


def struct_dict(m):
    """Every field of a ctypes struct: integers as they are, doubles as hex floats."""
    def conv(v):
        return float(v).hex() if isinstance(v, float) else int(v)
    out = {}
    for f, _ in m._fields_:
        v = getattr(m, f)
        out[f] = [conv(x) for x in v] if hasattr(v, "__len__") else conv(v)
    return out


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x, np.int16).tobytes()).hexdigest()


def record_level(pcm, rate, T, C, W):
    from mastering_amd import native
    from test_level import host_level
    ce = native.MMCeiling()
    y, m = host_level(pcm, rate, T, C, W, ce)
    return {"sha256": [sha(y)], "level": struct_dict(m), "ceilings": [struct_dict(ce)] if C else []}


def record_album(tracks, rate, T, C, W):
    from test_album import host_album_level
    ys, m, alb, tr, ce = host_album_level(tracks, rate, T, C, W)
    return {"sha256": [sha(y) for y in ys], "level": struct_dict(m), "album_r128": struct_dict(alb),
            "r128s": [struct_dict(r) for r in tr], "ceilings": [struct_dict(c) for c in ce] if C else []}


def record_all():
    out = {f"level/{name}": record_level(*case) for name, case in level_cases().items()}
    out.update({f"album/{name}": record_album(*case) for name, case in album_cases().items()})
    return out


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case(golden):
    assert set(golden["cases"]) == {f"level/{n}" for n in level_cases()} | {f"album/{n}" for n in album_cases()}
    statuses = {rec["level"]["status"] for rec in golden["cases"].values()}
    assert statuses >= {1, 2, 3, 5}  # reached, capped, saturated, unmeasurable


@pytest.mark.parametrize("name", sorted(f"level/{n}" for n in (
    "down", "up-idle", "stepped", "mono-boost", "saturated", "capped", "no-ceiling", "window-1", "short-no-ceiling",
    "silence-no-ceiling", "short-ceiling", "silence-ceiling", "empty", "mono-48k", "mono-short-w220", "mono-short-w1",
    "views-0", "views-1", "views-2")))
def test_mm_level_host_is_what_it_was(golden, name):
    got, want = record_level(*level_cases()[name.split("/")[1]]), golden["cases"][name]
    for k in want:
        assert got[k] == want[k], k
    assert set(got) == set(want)


@pytest.mark.parametrize("name", sorted(f"album/{n}" for n in (
    "cut", "hot-cut", "boost-2", "boost-3", "saturated", "mono", "no-ceiling", "unmeasurable", "one-cut", "one-boost",
    "one-no-ceiling", "one-short", "fates")))
def test_mm_album_level_host_is_what_it_was(golden, name):
    got, want = record_album(*album_cases()[name.split("/")[1]]), golden["cases"][name]
    for k in want:
        assert got[k] == want[k], k
    assert set(got) == set(want)
