#!/usr/bin/env python3
"""The loudness meter's kernels (k_hops, k_carry, k_true_peak, k_scale of atracdenc_amd/csrc/loudness.hip) through the CPU SIMT
harness (tools/emu), against the C restatement tests/host/loudness_cpu.c. Driver of tests/test_loudness_simt_harness.py, which
runs it in child processes because the harness reads EMU_STRICT, EMU_FENCE and EMU_ORDER when the library loads.

    run_emu_loudness.py [--nobuild] CASE ...

prints one `<what>: bad N` line per comparison (N = mismatching streams; 0 is a pass). The meter runs through the public
binding class with lib_path= the harness. CASES lists the cases."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import run_emu
import loudness_lib as L
from run_emu_decode import DevBuf, report
from atracdenc_amd.binding import AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, HipLoudness

EMU = run_emu.EMU
HOP = L.HOP


def compare(what, z, results, xs, true_peak, t0):
    """hop sums and every field of the results of all streams against the restatement"""
    bad_z = sum(not L.bits_equal(z[i], L.hops(xs[i])) for i in range(xs.shape[0]))
    bad_r = sum(not L.results_equal(results[i], L.measure(xs[i], true_peak)) for i in range(xs.shape[0]))
    report(f"{what} z", bad_z, t0)
    report(f"{what} results", bad_r)


def meter(channels):
    """the five signal kinds side by side, 7 hops and a partial one: one call, random cuts, reset() mid-stream; true peak on
    (and once off)"""
    T = 7 * HOP + 1234
    xs = np.stack([L.signal(k, T, channels, seed=10 * channels + i) for i, k in enumerate(L.KINDS)])
    rng = np.random.RandomState(50 + channels)
    m = HipLoudness(channels=channels, n_streams=len(L.KINDS), max_in=T, max_hops=8, true_peak=True, lib_path=EMU)
    t0 = time.time()
    z, res = L.run_split(m, xs, [T])
    compare(f"loudness ch{channels} one call", z, res, xs, True, t0)
    t0 = time.time()
    cuts = L.random_cuts(rng, T, 6)
    z, res = L.run_split(m, xs, cuts)   # (finish() has returned the meter to its start state)
    compare(f"loudness ch{channels} cuts {cuts}", z, res, xs, True, t0)
    t0 = time.time()
    m.process(xs[:, :HOP + 99])
    m.reset()
    z, res = L.run_split(m, xs, [3, 2 * HOP, 2 * HOP + 1, T])
    compare(f"loudness ch{channels} after reset", z, res, xs, True, t0)
    m.close()
    t0 = time.time()
    m = HipLoudness(channels=channels, n_streams=len(L.KINDS), max_in=T, max_hops=8, true_peak=False, lib_path=EMU)
    z, res = L.run_split(m, xs, [HOP, T])
    compare(f"loudness ch{channels} without true peak", z, res, xs, False, t0)
    m.close()


def edges():
    """caller-owned device buffers of exactly the input's size (under EMU_FENCE they end or begin at the guard page); calls
    shorter than the converter's filter, empty calls, a stream shorter than a hop, more lanes than one workgroup of k_hops
    holds and a last workgroup that is not full"""
    t0 = time.time()
    C, S, T = 2, 3, 2 * HOP + 500
    xs = np.stack([L.signal(k, T, C, seed=70 + i) for i, k in enumerate(("noise", "tone_dc", "sweep"))])
    m = HipLoudness(channels=C, n_streams=S, max_in=T, max_hops=2, true_peak=True, lib_path=EMU)
    at = 0
    for cut in (0, 5, 40, 100, HOP, HOP, T):
        piece = np.ascontiguousarray(xs[:, at:cut])
        if piece.shape[1]:
            src = DevBuf(piece.nbytes).write(piece)
            m.process_ptr(src.ptr, cut - at, AT3HIP_PCM_ON_DEVICE)
            src.free()
        else:
            m.process(piece)
        at = cut
    z = m.hops()
    compare("loudness exact device buffers, short and empty calls", z, m.finish(), xs, True, t0)
    t0 = time.time()
    z, res = L.run_split(m, xs[:, :777], [300, 777])   # no complete hop: peaks from k_carry and the flush alone
    compare("loudness shorter than a hop", z, res, np.ascontiguousarray(xs[:, :777]), True, t0)
    res = m.finish()   # nothing received
    report("loudness empty finish", sum(not L.results_equal(res[i], L.measure(xs[i, :0], True)) for i in range(S)))
    m.close()
    t0 = time.time()
    S, T = 23, 3 * HOP + 11   # 69 (stream, hop) pairs: mono 2 workgroups, the last one with 5 lanes
    xs = np.stack([L.signal(L.KINDS[i % 5], T, 1, seed=90 + i) for i in range(S)])
    m = HipLoudness(channels=1, n_streams=S, max_in=T, max_hops=3, lib_path=EMU)
    z, res = L.run_split(m, xs, [T])
    compare("loudness 23 mono streams", z, res, xs, False, t0)
    m.close()


def scale():
    """k_scale: bit-equal to numpy's float32 multiply; host memory, and caller-owned device buffers of exact size (lengths that
    take the float4 form and the scalar form), in place too"""
    t0 = time.time()
    bad = 0
    rng = np.random.RandomState(4)
    for C, S, n in ((2, 3, 1000), (1, 5, 333), (2, 2, 7), (1, 1, 4096)):
        xs = np.stack([L.signal(L.KINDS[i % 5], n, C, seed=30 + i) for i in range(S)])
        g = rng.uniform(0.1, 3.0, S).astype(np.float32)
        want = xs * g[:, None, None]
        m = HipLoudness(channels=C, n_streams=S, max_in=n, max_hops=1, lib_path=EMU)
        bad += int(not L.bits_equal(m.apply(xs, g), want))
        src, dst = DevBuf(xs.nbytes).write(xs), DevBuf(xs.nbytes)
        m.apply_ptr(src.ptr, n, g, dst.ptr, AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE)
        bad += int(not L.bits_equal(dst.read(np.float32, xs.shape), want))
        m.apply_ptr(src.ptr, n, g, src.ptr, AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE)   # in place
        bad += int(not L.bits_equal(src.read(np.float32, xs.shape), want))
        src.free()
        dst.free()
        m.close()
    report("loudness apply", bad, t0)


def domain(channels):
    """tests/float_domain_lib.py's streams (NaN, infinities, +-FLT_MAX, overflowing and subnormal samples) side by side, 1.2 s each, true peak
    on, one call and three: hop sums, every field of the results and apply's samples against the restatement of each stream alone"""
    import float_domain_lib as FD
    exp = FD.meter_expect(channels)
    for cuts in ((FD.METER_T,), FD.METER_CUTS):
        t0 = time.time()
        bad = FD.meter_bad(FD.meter_run(EMU, channels, cuts=cuts), exp)
        for what in ("z", "results", "apply"):
            report(f"loudness domain ch{channels} cuts {cuts} {what} {bad[what]}", len(bad[what]), t0)


CASES = {"domain:1": domain, "domain:2": domain, "meter:1": meter, "meter:2": meter, "edges": edges, "scale": scale}

if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    unknown = [n for n in names if n not in CASES]
    if unknown or not names:
        sys.exit(f"usage: run_emu_loudness.py [--nobuild] CASE ...; cases: {' '.join(CASES)}")
    if "--nobuild" not in sys.argv:
        run_emu.build(strict=True)
    os.environ.setdefault("EMU_STRICT", "1")
    for n in names:
        t = time.time()
        CASES[n](*(int(a) for a in n.split(":")[1:]))
        print(f"{n} done ({time.time() - t:.1f}s)", flush=True)
