"""The release-jump records' base rule (csrc/compressor.hip rec_base)
restated in Python and checked on the CPU.

A tile's record covers JB binades from its base.  The base was the binade of the
tile's largest M; it is now the band's fixed base e0fix = binade(the table's largest
M) - (JB - 1) whenever the tile's largest M reaches 2^e0fix (comp_rms_t then walks the
references while it holds the tile's M values), and the binade of the largest M below
that (comp_describe walks those).  Checked here, on the per-frame M of real band
signals:
  * every jump taken under the new rule lands bit for bit on the stepped state;
  * every (tile, true entry state) the old rule covers, the new rule covers;
  * the P_FULL high band has tiles under the per-tile branch (else it goes untested).
tests/test_envelope_jumps.py keeps modelling the definition (the old rule's describer
and the jump conditions, imported from there for the comparison).  The helpers that
build the records of a whole band are shared with tests/test_gpu_record_base.py,
which compares them with the device's, bit for bit."""
import functools
import math

import numpy as np
import pytest

import signals as S
from mastering_amd import design
from test_envelope_jumps import JB, MANT, _binade, _bits, _describe, _from, _jump, _step

RATE = 44100
TILE = design.choose_tile(design.pydub_frame(design.CHUNK_MS, RATE))  # 225
NAN_BITS = 0x7FF8000000000000


def e0fix_of(table):
    """The band's fixed record base from its M table (the last row is the largest M)."""
    return _binade(float(table[32768])) - (JB - 1)


def rec_base(mx, e0fix):
    e = _binade(mx)
    return e0fix if e >= e0fix else e


def describe_new(M, R, e0fix):
    """One active tile's record under the new rule: (max M, base, q[2 JB])."""
    mx = max(M)
    e0 = rec_base(mx, e0fix)
    r0 = [_from(((e0 + k // 2 + 1023) << 52) | (MANT - 63 + k % 2)) for k in range(2 * JB)]
    r = list(r0)
    for m in M:
        dec = m / R
        r = [x - dec for x in r]
    q = []
    for k in range(2 * JB):
        rb = _bits(r[k])
        ok = (rb >> 52) == e0 + k // 2 + 1023 and (rb & MANT) != 0
        q.append(r0[k] - r[k] if ok else math.nan)
    return mx, e0, q


def band_records(M, R, e0fix, tile=TILE):
    """Every active tile of one chunk's band, vectorised over tiles: (tile indices,
    largest M, bases, records [n, 2 JB] as uint64 bit patterns, NaN = NAN_BITS)."""
    M = np.asarray(M, np.float64)
    nt = -(-M.shape[0] // tile)
    Mp = np.zeros(nt * tile)
    Mp[:M.shape[0]] = M  # rows past a partial last tile: M = 0, d = 0
    Mt = Mp.reshape(nt, tile)
    mx = Mt.max(axis=1)
    live = np.flatnonzero(mx > 0.0)
    Mt, mx = Mt[live], mx[live]
    eb = np.frexp(mx)[1] - 1
    base = np.where(eb >= e0fix, e0fix, eb).astype(np.int64)
    k = np.arange(2 * JB)
    bits = ((base[:, None] + k[None, :] // 2 + 1023).astype(np.uint64) << np.uint64(52)) | \
        (np.uint64(MANT - 63) + (k[None, :] % 2).astype(np.uint64))
    r0 = bits.view(np.float64)
    r = r0.copy()
    D = Mt / R  # correctly rounded, as div_cr
    for n in range(tile):
        r = r - D[:, n:n + 1]
    rb = r.view(np.uint64)
    ok = ((rb >> np.uint64(52)) == (bits >> np.uint64(52))) & ((rb & np.uint64(MANT)) != 0)
    q = np.where(ok, (r0 - r).view(np.uint64), np.uint64(NAN_BITS))
    return live, mx, base, q


@functools.lru_cache(maxsize=None)
def bands_of(source):
    """[(M per frame, attack frames, release frames, table)] per band: 2 s of the
    bench's pink noise (track 0) under P_FULL / P_HOT, or the staircase band inputs."""
    if source == "staircase":
        hold = int(S.SECONDS * S.RATE) // 8
        out = []
        for x, st in zip(S.staircase_bands(1, hold=hold)[:2], S.band_settings()):
            b = S.band_structure(x, S.RATE, *st, TILE)
            out.append((b["M"], b["attack_frames"], b["release_frames"],
                        design.max_att_table(float(st[0]), float(st[1]))[0]))
        return out
    from mastering_amd.synth import pink_noise_pcm16
    params = {"full": S.P_FULL, "hot": S.P_HOT}[source]
    pcm = pink_noise_pcm16(2 * RATE, RATE, 2, track=0)
    st = S.structure(pcm, RATE, params)
    return [(b["M"], b["attack_frames"], b["release_frames"], design.max_att_table(float(t), float(r))[0])
            for b, (t, r, _, _) in zip(st["chunks"][0], S.band_settings(params))]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("source", ["full", "hot", "staircase"])
def test_new_base_rule(source):
    jumps = checked = per_tile = fixed = 0
    for bi, (M, A, R, table) in enumerate(bands_of(source)):
        e0fix = e0fix_of(table)
        top = float(table[32768])
        traj = [0.0]
        for m in M:
            traj.append(_step(traj[-1], float(m), A, R))
        assert max(traj) <= top  # no state exceeds the table's largest M
        live, mxs, bases, q = band_records(M, R, e0fix)
        for i, t in enumerate(live):
            seg = [float(v) for v in M[t * TILE:(t + 1) * TILE]]
            new = describe_new(seg, R, e0fix)
            old = _describe(seg, R)
            # the vectorised builder (shared with the GPU test) is the per-tile restatement
            assert new[0] == mxs[i] and new[1] == bases[i]
            assert [_bits(v) if v == v else NAN_BITS for v in new[2]] == [int(v) for v in q[i]]
            if new[1] == e0fix:
                fixed += 1
            else:
                per_tile += 1
                assert new[1] == old[1] and [_bits(v) for v in new[2]] == [_bits(v) for v in old[2]]
            true = traj[t * TILE]
            # coverage: what the old rule jumps from the true entry state, the new rule jumps
            xo, xn = _jump(old, true), _jump(new, true)
            assert xo is None or xn == xo, (bi, t, true, xo, xn)
            # exactness: the true state, its neighbours, states in the record's other binades
            for att in (true, math.nextafter(true, math.inf), math.nextafter(true, -math.inf), true * 1.5,
                        new[0] * 1.0001, new[0] * 2.01, new[0] * 4.3, top, top * 0.5, top * 0.124):
                checked += 1
                x = _jump(new, att)
                if x is None:
                    continue
                jumps += 1
                y = att
                for m in seg:
                    y = _step(y, m, A, R)
                assert x == y, (bi, t, att, x, y)
        if source == "full" and bi == 2:
            print(f"P_FULL high band: {per_tile_band(bases, e0fix)} of {len(live)} active tiles under the per-tile branch")
            assert per_tile_band(bases, e0fix) >= 1
    print(f"{source}: {jumps} of {checked} probes jumped; {fixed} tiles at the fixed base, {per_tile} per tile")
    assert jumps > 0


def per_tile_band(bases, e0fix):
    return int(np.count_nonzero(np.asarray(bases) != e0fix))
