"""A reference and a model of the look-back IIR operator (csrc/lookback.h behind
mm_op_sosfilt), plus the cases tests/test_iir_model.py (CPU) and
tests/test_gpu_iir_seams.py (GPU) share.

sos_reference   the DF2T cascade as a sequential loop in np.longdouble (80-bit on
                x86): what the operator is meant to compute, to 11 more bits than
                the device carries.
lookback_model  an f64 numpy restatement of what lookback.h computes: the tiles'
                zero-state end states, the block-local Kogge-Stone scan, the block
                aggregates, the block carry (one of the two extremes the kernel's
                timing can produce) and Phi_T^t C_b from the bits of t, then every
                tile re-run from its carry-in.  It builds its one-frame matrix and
                every power from the five coefficients itself (nothing from
                mastering_amd.design), so an error in design's tables shows as a
                kernel error against it.
tolerance       the gate: 8 x the larger model path's error against the reference,
                with a floor of 64 x 2^-52 x max|reference|.

Both are causal and tile-aligned at frame 0, so one evaluation at the longest size
serves every shorter size by slicing (cached below; the arrays are read-only).
"""
import functools

import numpy as np

LB_THREADS = 256   # csrc/lookback.h
LB_WIN = 64
OPS_TILES = 16     # csrc/ops.hip: tiles per block of the two transposes


# ------------------------------------------------------------------ reference
def _cascade(x, sections, round_f32, dtype):
    """Outputs of every prefix of the cascade: [len(sections)][N, C] in `dtype`."""
    x = np.asarray(x)
    cols = x.reshape(x.shape[0], -1).astype(dtype)
    n, c = cols.shape
    sec = [[dtype(v) for v in s] for s in sections]
    z = [[np.zeros(c, dtype), np.zeros(c, dtype)] for _ in sec]
    outs = [np.empty((n, c), dtype) for _ in sec]
    for i in range(n):
        v = cols[i]
        for k, (b0, b1, b2, a1, a2) in enumerate(sec):
            z0, z1 = z[k]
            y = b0 * v + z0
            z[k][0] = (b1 * v - a1 * y) + z1
            z[k][1] = b2 * v - a2 * y
            if round_f32:
                y = y.astype(np.float32).astype(dtype)
            outs[k][i] = y
            v = y
    return outs


def sos_reference(x, sections, round_f32=False, dtype=np.longdouble):
    """DF2T cascade (sections of b0 b1 b2 a1 a2, a0 = 1) over each channel of x [N]
    or [N, C], zero initial state, sequentially in `dtype`.  round_f32: every
    section's output is rounded to float32 before the next one (the state update
    uses the unrounded output, as iir_op_pass<R32> and lfilter-then-write-back do)."""
    x = np.asarray(x)
    return _cascade(x, sections, round_f32, dtype)[-1].reshape(x.shape)


# ---------------------------------------------------------------------- model
def _step_matrix(sections):
    """One zero-input frame of the cascade as a matrix on the state (z0, z1 per
    section, in section order), from row functionals: u = the section's input."""
    d = 2 * len(sections)
    A = np.zeros((d, d))
    u = np.zeros(d)
    for s, (b0, b1, b2, a1, a2) in enumerate(sections):
        e0, e1 = np.zeros(d), np.zeros(d)
        e0[2 * s], e1[2 * s + 1] = 1.0, 1.0
        y = b0 * u + e0
        A[2 * s] = b1 * u - a1 * y + e1
        A[2 * s + 1] = b2 * u - a2 * y
        u = y
    return A


def _mpow(M, n):
    out = np.eye(M.shape[0], dtype=M.dtype)
    sq = M.copy()
    while n:
        if n & 1:
            out = out @ sq
        n >>= 1
        if n:
            sq = sq @ sq
    return out


def _run_tiles(xt, sections, state, round_f32, want_out):
    """xt [T, G, C] frames of every tile, state [G, C, D] on entry (modified in
    place to the state at the tiles' ends); scipy's operation order in f64."""
    out = np.empty_like(xt) if want_out else None
    for n in range(xt.shape[0]):
        v = xt[n]
        for s, (b0, b1, b2, a1, a2) in enumerate(sections):
            z0, z1 = state[..., 2 * s], state[..., 2 * s + 1]
            y = b0 * v + z0
            state[..., 2 * s] = (b1 * v - a1 * y) + z1
            state[..., 2 * s + 1] = b2 * v - a2 * y
            if round_f32:
                y = y.astype(np.float32).astype(np.float64)
            v = y
        if want_out:
            out[n] = v
    return out


def _mv(M, v):
    """M v over the last axis of v."""
    return np.einsum("rk,...k->...r", M, v)


def lookback_model(x, sections, T, tpb, path, round_f32=False, mutate=None):
    """What lookback.h computes for the cascade over x [N] or [N, C] with T-frame
    tiles and tpb tiles per workgroup, in float64.  path: "inclusive" (every block
    finds its predecessor's inclusive prefix) or "aggregates" (every block sums
    Phi_B^i agg_{b-1-i} back to the line start, in windows of 64 with the Phi_B^64
    update).  mutate (the mutation check only): "blk_pow" uses Phi_B^(i+1) for
    Phi_B^i, "swap" hands the two channels each other's block carry, "t_plus_1"
    applies Phi_T^(t+1) C_b."""
    assert path in ("inclusive", "aggregates") and mutate in (None, "blk_pow", "swap", "t_plus_1")
    x = np.asarray(x, np.float64)
    shape = x.shape
    cols = x.reshape(shape[0], -1)
    N, C = cols.shape
    sections = [tuple(float(v) for v in s) for s in sections]
    D = 2 * len(sections)
    G = -(-N // T)
    nb = -(-G // tpb)
    xt = np.zeros((nb * tpb * T, C))
    xt[:N] = cols
    xt = xt.reshape(nb * tpb, T, C).transpose(1, 0, 2)  # [T, tiles, C]

    A = _step_matrix(sections)
    tile_pow = [_mpow(A, T)]
    while (1 << len(tile_pow)) < tpb:
        tile_pow.append(tile_pow[-1] @ tile_pow[-1])
    phi_b = _mpow(tile_pow[0], tpb)
    blk_pow = [np.eye(D)]
    for _ in range(LB_WIN + 1):
        blk_pow.append(blk_pow[-1] @ phi_b)

    # each tile's zero-state end state; lanes past the signal contribute zeros
    z = np.zeros((nb * tpb, C, D))
    _run_tiles(xt, sections, z, round_f32, False)
    z[G:] = 0.0
    v = z.reshape(nb, tpb, C, D).copy()
    f = np.zeros((nb, tpb), bool)
    f[0, 0] = True  # the line start
    # 1. block-local inclusive scan (Kogge-Stone; a flagged tile takes nothing more)
    for k in range(len(tile_pow)):
        dist = 1 << k
        if dist >= tpb:
            break
        add = _mv(tile_pow[k], v[:, :-dist])
        take = ~f[:, dist:]
        nv, nf = v.copy(), f.copy()
        nv[:, dist:] += np.where(take[..., None, None], add, 0.0)
        nf[:, dist:] = np.where(take, f[:, :-dist], f[:, dist:])
        v, f = nv, nf
    sp = np.zeros_like(v)  # local exclusive prefix
    sp[:, 1:] = v[:, :-1]
    # 2. aggregates; block 0 holds the line start, so its aggregate is its prefix
    agg = v[:, -1]  # [nb, C, D]
    # 3. block carry
    cb = np.zeros((nb, C, D))
    incl = np.zeros((nb, C, D))
    incl[0] = agg[0]
    sh = 1 if mutate == "blk_pow" else 0
    bp = np.stack(blk_pow)
    for b in range(1, nb):
        if path == "inclusive":
            cb[b] = _mv(blk_pow[sh], incl[b - 1])
        else:
            pw = np.eye(D)
            pub = agg.copy()
            pub[0] = incl[0]  # what lane i finds at block j: aggregates, the prefix at the line start
            w = 0
            while True:
                hi = b - 1 - w * LB_WIN  # lane 0's block
                nl = min(LB_WIN, hi + 1)
                terms = np.zeros((LB_WIN, C, D))
                terms[:nl] = np.einsum("lrk,lck->lcr", bp[sh:sh + nl], pub[hi - nl + 1:hi + 1][::-1])
                h = LB_WIN
                while h > 1:  # the wave's butterfly sum
                    h //= 2
                    terms = terms[:h] + terms[h:2 * h]
                cb[b] += _mv(pw, terms[0])
                if hi < LB_WIN:
                    break
                pw = pw @ blk_pow[LB_WIN]
                w += 1
        incl[b] = _mv(blk_pow[1], cb[b]) + agg[b]
    if mutate == "swap" and C == 2:
        cb = cb[:, ::-1].copy()
    # 4. Phi_T^t C_b from the bits of t
    tt = np.arange(tpb) + (1 if mutate == "t_plus_1" else 0)
    pows = tile_pow + [tile_pow[-1] @ tile_pow[-1]]
    cv = np.repeat(cb[1:, None], tpb, axis=1)  # [nb - 1, tpb, C, D]
    for k, P in enumerate(pows):
        sel = ((tt >> k) & 1).astype(bool)
        cv[:, sel] = _mv(P, cv[:, sel])
    s = sp.copy()
    s[1:] += cv
    # every tile again from its carry-in
    state = s.reshape(nb * tpb, C, D)
    out = _run_tiles(xt, sections, state, round_f32, True)  # [T, tiles, C]
    return out.transpose(1, 0, 2).reshape(nb * tpb * T, C)[:N].reshape(shape)


def tolerance(ref, e_model):
    """The gate of the R32-off cases: 8 x the model's own error, not below 64 ulp of
    the reference's peak."""
    return max(8.0 * e_model, 64.0 * 2.0 ** -52 * float(np.max(np.abs(ref))))


# ---------------------------------------------------------------------- cases
TILES = (1, 3, 4, 125)
G6 = 10.0 ** (6.0 / 20.0)
MIX = ((1.0, G6 - 1.0), (G6, 1.0 - G6))  # mm_op_sosfilt_mix (a, c)


def block_frames(T, ch):
    return T * LB_THREADS // ch


def sizes(T, ch):
    B = block_frames(T, ch)
    if T == 125:
        return [B - 1, B + 1, 3 * B + 5]
    raw = [1, T - 1, T, T + 1, OPS_TILES * T, OPS_TILES * T + 1, B - 1, B, B + 1, 2 * B + T + 1, 65 * B + 3]
    return sorted({n for n in raw if n > 0})


MAX_FRAMES = max(max(sizes(T, ch)) for T in TILES for ch in (1, 2))  # 96005


def filters():
    """name -> sections, all from mastering_amd.design (the product's coefficients)."""
    from mastering_amd import EQ_PRESETS, design
    eq = design.eq_sections(44100, EQ_PRESETS["techno"])
    assert len(eq) == 4
    out = {f"techno{k}": eq[:k] for k in (1, 2, 3, 4)}
    out["kweight"] = design.kweight_sections(48000)
    out["shelf20"] = [design.shelf_section(192000, 20, 12, "low", 0.707)]
    return out


# (filter, round_f32): the six the issue names, and the techno prefixes with the f32
# write-back so that every (NS, CH, R32) instantiation of iir_op_kernel runs
R32_OFF = ("techno1", "techno2", "techno3", "techno4", "kweight", "shelf20")
R32_ON = ("kweight", "techno1", "techno3", "techno4")



def seam_cases():
    """(filter, round_f32, T, ch) of the seam tests.  T = 4 and T = 125 meet every
    filter; T = 1 and T = 3 the longest cascade, the ill-conditioned shelf and the
    K-weighting with and without the write-back."""
    out = []
    for ch in (1, 2):
        for T in (4, 125):
            out += [(name, False, T, ch) for name in R32_OFF] + [(name, True, T, ch) for name in R32_ON]
        for T in (1, 3):
            out += [("techno4", False, T, ch), ("shelf20", False, T, ch), ("kweight", False, T, ch),
                    ("kweight", True, T, ch)]
    return out


def runs(case):
    """(signal, float32 input) of one case: noise in both input types (the float64
    noise uses all 53 bits), DC and the impulse in one each.  The K-weighting with the
    write-back takes noise only: its high-pass lets DC and the impulse decay into the
    recurrence's own rounding noise, where the f64 and the long-double recurrence
    round to different f32 values (92772 of 96005 samples for DC), so there is no
    reference to hold a sample against."""
    name, r32, _, ch = case
    out = [("noise", True), ("noise", False)]
    if not (r32 and name == "kweight"):
        out += [("dc", False), ("impulse", True)]
    return out + [("noise_silence", True)] if ch == 2 else out


def case_id(case):
    name, r32, T, ch = case
    return f"{name}{'-r32' if r32 else ''}-T{T}-ch{ch}"


# base columns every signal is made of; impulses are the impulse response shifted
BASE = ("noiseA32", "noiseB32", "noiseA64", "noiseB64", "dc", "imp")


@functools.lru_cache(maxsize=None)
def base_signals():
    # Seeds for which the f64 and the long-double recurrence with the f32 write-back
    # agree on every sample of every R32 case (searched among 20260101 .. 20260140; about
    # one seed in four does; tests/test_iir_model.py asserts it)
    def noise(seed):
        return np.random.default_rng(seed).uniform(-1.0, 1.0, MAX_FRAMES)
    a, b32, b64 = noise(20260125), noise(20260104), noise(20260105)
    imp = np.zeros(MAX_FRAMES)
    imp[0] = 1.0
    cols = [a.astype(np.float32).astype(np.float64), b32.astype(np.float32).astype(np.float64), a, b64,
            np.ones(MAX_FRAMES), imp]
    x = np.stack(cols, axis=1)
    x.setflags(write=False)
    return x


def _shift(col, p):
    out = np.zeros_like(col)
    out[p:] = col[:len(col) - p]
    return out


def _compose(base, sig, ch, f32, p):
    """A signal's channels from base columns [N, len(BASE)] (of the input, or of a
    filter's response to it: shifting an impulse commutes with the filter bit for bit,
    the f32 write-back included, and so does halving DC, whose responses stay far from
    the subnormals)."""
    na, nb_ = (base[:, 0], base[:, 1]) if f32 else (base[:, 2], base[:, 3])
    if sig == "noise":
        cols = [na, nb_]
    elif sig == "dc":
        cols = [base[:, 4], 0.5 * base[:, 4]]
    elif sig == "impulse":  # (not a scaled copy: halving is inexact on f32 subnormals of the decayed tail)
        cols = [_shift(base[:, 5], p), _shift(base[:, 5], p - 1)]
    elif sig == "noise_silence":
        cols = [na, np.zeros_like(na)]
    else:
        raise KeyError(sig)
    return cols[0].copy() if ch == 1 else np.stack(cols, axis=1)


SIGNALS = ("noise", "dc", "impulse", "noise_silence")


def signal(sig, T, ch, f32):
    """The input [MAX_FRAMES] or [MAX_FRAMES, 2] (float64 values; float32-exact when
    f32).  The impulse sits at frame B - 1 (right channel: B - 2): everything after it
    is carried by the look-back alone."""
    return _compose(base_signals(), sig, ch, f32, block_frames(T, ch) - 1)


def _cascade_both(x, sections):
    """_cascade in long double with and without the f32 write-back in one loop (row 0
    of the state plain, row 1 rounded): ([k][N, C] plain, [k][N, C] rounded)."""
    ld = np.longdouble
    cols = np.asarray(x).astype(ld)
    n, c = cols.shape
    sec = [[ld(v) for v in s] for s in sections]
    z0 = [np.zeros((2, c), ld) for _ in sec]
    z1 = [np.zeros((2, c), ld) for _ in sec]
    plain = [np.empty((n, c), ld) for _ in sec]
    rounded = [np.empty((n, c), ld) for _ in sec]
    for i in range(n):
        v = cols[i]
        for k, (b0, b1, b2, a1, a2) in enumerate(sec):
            y = b0 * v + z0[k]
            z0[k] = (b1 * v - a1 * y) + z1[k]
            z1[k] = b2 * v - a2 * y
            y[1] = y[1].astype(np.float32)
            plain[k][i] = y[0]
            rounded[k][i] = y[1]
            v = y
    return plain, rounded


@functools.lru_cache(maxsize=None)
def _reference_base(fam):
    outs = _cascade_both(base_signals(), filters()[fam])
    for o in outs[0] + outs[1]:
        o.setflags(write=False)
    return outs


@functools.lru_cache(maxsize=None)
def _f64_base(name, round_f32):
    """The sequential recurrence in f64: scipy.signal.sosfilt, whose bits the f64
    instance of _cascade reproduces (tests/test_iir_model.py), a section at a time
    with the write-back between them when round_f32."""
    from scipy.signal import sosfilt
    y = base_signals()
    for b0, b1, b2, a1, a2 in filters()[name]:
        y = sosfilt(np.array([[b0, b1, b2, 1.0, a1, a2]]), y, axis=0)
        if round_f32:
            y = y.astype(np.float32).astype(np.float64)
    y.setflags(write=False)
    return y


def reference(name, round_f32, sig, T, ch, f32, dtype=np.longdouble):
    """The sequential filter's output for a signal [MAX_FRAMES] or [MAX_FRAMES, 2], in
    long double (the reference) or float64 (scipy's recurrence)."""
    if dtype == np.float64:
        base = _f64_base(name, round_f32)
    else:
        k = int(name[-1]) if name.startswith("techno") else len(filters()[name])
        base = _reference_base("techno4" if name.startswith("techno") else name)[int(round_f32)][k - 1]
    return _compose(base, sig, ch, f32, block_frames(T, ch) - 1)


@functools.lru_cache(maxsize=None)
def _model_base(name, T, tpb, path):
    m = lookback_model(base_signals(), filters()[name], T, tpb, path)
    m.setflags(write=False)
    return m


def model(name, path, sig, T, ch, f32):
    """The model's output for a signal.  The model is linear in the input only up to
    rounding, so the impulse and the stereo pairs are run as they are, not composed."""
    if sig in ("noise", "noise_silence") and ch == 1:
        return _model_base(name, T, LB_THREADS, path)[:, 0 if f32 else 2]
    if sig == "dc" and ch == 1:
        return _model_base(name, T, LB_THREADS, path)[:, 4]
    return _model_signal(name, path, sig, T, ch, f32)


@functools.lru_cache(maxsize=None)
def _model_signal(name, path, sig, T, ch, f32):
    n = max(sizes(T, ch))
    m = lookback_model(signal(sig, T, ch, f32)[:n], filters()[name], T, LB_THREADS // ch, path)
    m.setflags(write=False)
    return m


def err(a, ref):
    return float(np.max(np.abs(np.asarray(a, np.longdouble) - ref)))
