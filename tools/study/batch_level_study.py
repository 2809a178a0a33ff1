"""DESIGN 4l's measurement: mm_batch_level_device against one mm_level_device call a track.

The album of DESIGN 4k (12 tracks of 3 min, 44.1 kHz, stereo int16, mastered as a batch) is
levelled to one target under -1 dBTP by the batch level (every launch over all tracks) and, on
copies of the same buffers, by twelve mm_level_device calls (the single-track path).  The two
are alternated in one process; wall time is a host clock around the synchronous calls, kernel
time is mm_timing's events in rounds of their own.  The outputs and the mm_level of every track
are compared for equality.  Prints one JSON line and, with --out, writes it to a file.

    python tools/study/batch_level_study.py [--tracks 12] [--seconds 180] [--rounds 10] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "python-audio-mastering_amd"))

PARAMS = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0, "saturation": 30, "width": 1.3,
          "multiband": True, "lufs": -14.0}


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=12)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--target", type=float, default=-14.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from mastering_amd import Job, design, engine, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16

    rate, n = 44100, a.tracks
    frames = int(a.seconds * rate)
    pcms = [pink_noise_pcm16(frames, rate, 2, track=t) for t in range(n)]
    ctx = native.context(0)
    jobs = [Job(frames, rate, 2, PARAMS) for _ in range(n)]
    for j in jobs:
        j.job.in_kind = native.MM_IN_I16
    xs = [torch.from_numpy(p).cuda() for p in pcms]
    src = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
    torch.cuda.synchronize()
    master_batch(ctx, jobs, [x.data_ptr() for x in xs], [s.data_ptr() for s in src])
    del xs

    fr = [j.frames_proc for j in jobs]
    c_frames = (ctypes.c_int64 * n)(*fr)
    clu, C, W = design.level_clu(a.target), design.ceiling_q28(-1.0), design.ceiling_window(rate)
    c_clu, c_C = (ctypes.c_int32 * n)(*[clu] * n), (ctypes.c_int32 * n)(*[C] * n)
    sos = engine.kweight_sos(rate)
    A = [torch.empty_like(s) for s in src]
    B = [torch.empty_like(s) for s in src]

    def refill(dst):
        for d, s in zip(dst, src):
            d.copy_(s)
        torch.cuda.synchronize()

    def run_batch():
        ctx.check(ctx.lib.mm_batch_level_device(ctx.ptr, engine._pointers([t.data_ptr() for t in A]), native.MM_OUT_I16,
                                                c_frames, n, 2, rate, sos, c_clu, c_C, W), "mm_batch_level_device")

    singles = [native.MMLevel() for _ in range(n)]

    def run_singles():
        for t in range(n):
            ctx.check(ctx.lib.mm_level_device(ctx.ptr, ctypes.c_void_p(B[t].data_ptr()), native.MM_OUT_I16, fr[t], 2, rate,
                                              sos, clu, C, W, ctypes.byref(singles[t]), None), "mm_level_device")

    def timed(fn, dst):
        refill(dst)
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):  # warm both paths (buffers, tables)
        timed(run_batch, A)
        timed(run_singles, B)
    timed(run_batch, A)
    lv = engine.levels(ctx, n)
    timed(run_singles, B)
    raw = lambda m: ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m))  # noqa: E731
    equal = all(torch.equal(x, y) for x, y in zip(A, B)) and all(raw(p) == raw(q) for p, q in zip(lv, singles))

    wall_b, wall_s = [], []
    for _ in range(a.rounds):
        wall_b.append(timed(run_batch, A))
        wall_s.append(timed(run_singles, B))

    def kernels(fn, dst):
        refill(dst)
        ctx.timing(True)
        try:
            fn()
            st = ctx.kernel_stats()
        finally:
            ctx.timing(False)
        return sum(v[0] for v in st.values()), {k: [round(v[0], 4), v[1]] for k, v in st.items()}

    kb, ks, last_b, last_s = [], [], None, None
    for _ in range(max(4, a.rounds // 2)):
        ms, last_b = kernels(run_batch, A)
        kb.append(ms)
        ms, last_s = kernels(run_singles, B)
        ks.append(ms)

    res = {"tracks": n, "frames": fr[0], "target_lufs": a.target, "ceiling_dbtp": -1.0, "outputs_equal": bool(equal),
           "passes_batch_lockstep": max(m.passes for m in lv), "passes_per_track": [m.passes for m in singles],
           "status": [native.LEVEL_STATUS[m.status] for m in singles],
           "wall_ms": {"batch": summary(wall_b), "per_track_calls": summary(wall_s)},
           "kernel_ms": {"batch": summary(kb), "per_track_calls": summary(ks)},
           "kernels_batch": last_b, "kernels_per_track_calls": last_s}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
