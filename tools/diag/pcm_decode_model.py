"""CPU model of pcm_decode_kernel's addressing (csrc/decode.hip), statement for statement:
which aligned dwords a launch loads and which outputs it stores, for every sample count
of tests/test_gpu_hires.py x input byte phase x output 16-byte phase, both widths.
Asserts that the dwords loaded are exactly the aligned dwords holding at least one input
byte (nothing before, nothing past the end, 16-byte loads only where all 16 bytes are
such dwords), that every output index in [0, n) is stored exactly once and nothing else,
and that the values are the left-justified samples.  Usage: python tools/diag/pcm_decode_model.py"""
import numpy as np

SPAN, THREADS, QUADS = 4096, 256, 4  # DEC_SPAN, DEC_THREADS, DEC_QUADS


def alignbyte(hi, lo, sh):
    return (((hi << 32) | lo) >> (8 * sh)) & 0xFFFFFFFF


def launch(bps, ia, n, oa, mem_base, mem):
    dwords = 3 + bps * (SPAN // 4) + 1
    chunks = (dwords + 3) // 4
    hs = (oa >> 2) & 3
    lo, hi = ia & ~3, (ia + n * bps + 3) & ~3
    vb = ia - bps * hs
    p = vb & 3
    spans = (hs + n + SPAN - 1) // SPAN
    loaded, wide, out = set(), 0, {}

    def load(a):
        assert lo <= a and a + 4 <= hi and a % 4 == 0, (a, lo, hi)
        loaded.add(a)
        return int.from_bytes(bytes(mem[a - mem_base:a - mem_base + 4]), "little")

    for s in range(spans):  # (the grid-stride loop: every span once)
        b0 = vb + s * SPAN * bps
        a0 = b0 & ~15
        lds = [0] * (chunks * 4)
        for k in range(chunks):
            a = a0 + 16 * k
            if a >= lo and a + 16 <= hi:
                assert a % 16 == 0
                wide += 1
                for d in range(4):
                    lds[4 * k + d] = load(a + 4 * d)
            else:
                for d in range(4):
                    if a + 4 * d >= lo and a + 4 * d + 4 <= hi:
                        lds[4 * k + d] = load(a + 4 * d)
        dw = (b0 - a0) >> 2
        for ql in range(QUADS * THREADS):
            i = s * SPAN + 4 * ql - hs
            w = lds[dw + bps * ql:dw + bps * ql + 4]
            assert len(w) == 4  # inside the stage
            if bps == 3:
                d0, d1, d2 = alignbyte(w[1], w[0], p), alignbyte(w[2], w[1], p), alignbyte(w[3], w[2], p)
                v = [(d0 << 8) & 0xFFFFFFFF, (alignbyte(d1, d0, 3) << 8) & 0xFFFFFFFF,
                     (alignbyte(d2, d1, 2) << 8) & 0xFFFFFFFF, d2 & 0xFFFFFF00]
            else:
                v = w
            for e in range(4):
                if 0 <= i + e < n:
                    assert i + e not in out
                    out[i + e] = v[e] - (1 << 32) if v[e] >> 31 else v[e]
    return loaded, wide, out, lo, hi


def main():
    rng = np.random.default_rng(0)
    cases = 0
    for bps in (3, 4):
        for n in (1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3):
            for phase in ((0, 1, 2, 3) if bps == 3 else (0,)):
                for hs in range(4):
                    base = 1 << 20
                    mem = rng.integers(0, 256, bps * n + 64, dtype=np.uint8)
                    ia = base + 16 + phase
                    loaded, wide, out, lo, hi = launch(bps, ia, n, (1 << 24) + 4 * hs, base, mem)
                    assert loaded == set(range(lo, hi, 4)), (bps, n, phase, hs)
                    assert wide >= (hi - lo) // 16 - 1, (bps, n, phase, hs)  # all but the ends are 16-byte loads
                    raw = mem[16 + phase:16 + phase + bps * n].astype(np.int64).reshape(n, bps)
                    if bps == 3:
                        want = raw[:, 0] << 8 | raw[:, 1] << 16 | raw[:, 2] << 24
                    else:
                        want = raw[:, 0] | raw[:, 1] << 8 | raw[:, 2] << 16 | raw[:, 3] << 24
                    want = np.where(want >= 1 << 31, want - (1 << 32), want)
                    assert sorted(out) == list(range(n)) and all(out[i] == want[i] for i in range(n)), (bps, n, phase, hs)
                    cases += 1
    print(f"pcm_decode_model: {cases} launches, loads and stores as specified")


if __name__ == "__main__":
    main()
