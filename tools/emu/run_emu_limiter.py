#!/usr/bin/env python3
"""The look-ahead limiter's kernels (k_limit_detect, k_limit_gain, k_limit_carry, k_limit_init of
atracdenc_amd/csrc/loudness_limit.hpp) through the CPU SIMT harness (tools/emu), against the C restatement
tests/host/limiter_cpu.c. Driver of tests/test_limiter_simt_harness.py, which runs it in child processes because the harness
reads EMU_STRICT, EMU_FENCE and EMU_ORDER when the library loads.

    run_emu_limiter.py [--nobuild] CASE ...

prints one `<what>: bad N` line per comparison (N = mismatching streams; 0 is a pass). CASES lists the cases."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import run_emu
import limiter_lib as LM
from run_emu_decode import DevBuf, report
from atracdenc_amd.binding import AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, HipLoudness

EMU = run_emu.EMU


def parity(channels, true_peak):
    """limiter_lib.batch(): one call, the cuts of limiter_lib.cuts_for, a second run on the same context, 16-bit input"""
    xs = LM.batch(channels, true_peak)
    want = LM.expect(channels, true_peak)
    S, T = xs.shape[:2]
    rng = np.random.RandomState(30 + channels + 2 * true_peak)
    m = HipLoudness(channels=channels, n_streams=S, max_in=T, max_hops=1, lib_path=EMU)
    for what, cuts, s16 in (("one call", [T], False), ("cuts", LM.cuts_for(rng, T, true_peak), False), ("s16 cuts", [T // 3, T], True)):
        t0 = time.time()
        y, st = LM.run_engine(m, xs, LM.GAINS, LM.CEIL, true_peak, cuts, s16)
        report(f"limiter ch{channels} tp{true_peak} {what} {cuts if len(cuts) < 4 else len(cuts)}", len(LM.bad_streams(y, st, *want)), t0)
    m.close()


def edges():
    """caller-owned device buffers of exactly the call's size (under EMU_FENCE they end or begin at the guard page), for the
    input, the output and the flush, stereo with the true-peak detector and mono with the sample detector"""
    for channels, true_peak in ((2, True), (1, False)):
        t0 = time.time()
        xs = LM.batch(channels, true_peak)
        S, T = xs.shape[:2]
        m = HipLoudness(channels=channels, n_streams=S, max_in=T, max_hops=1, lib_path=EMU)
        m.limit_start(LM.GAINS, LM.CEIL, true_peak)
        d, at, got = LM.delay(true_peak), 0, []
        for cut in (40, 300, LM.TILE + 5, T):
            piece = np.ascontiguousarray(xs[:, at:cut])
            n = max(0, cut - d) - max(0, at - d)
            src, dst = DevBuf(piece.nbytes).write(piece), DevBuf(max(4, S * n * channels * 4))
            assert m.limit_ptr(src.ptr, cut - at, dst.ptr, AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE) == n
            m.sync()
            got.append(dst.read(np.float32, (S, n, channels)) if n else np.zeros((S, 0, channels), np.float32))
            src.free(); dst.free()
            at = cut
        dst = DevBuf(S * d * channels * 4)
        assert m.limit_flush_ptr(dst.ptr, AT3HIP_OUT_ON_DEVICE) == d
        m.sync()
        got.append(dst.read(np.float32, (S, d, channels)))
        dst.free()
        st = [(s.min_sum, s.n_limited) for s in m.limit_stats()]
        m.close()
        report(f"limiter exact device buffers ch{channels} tp{true_peak}", len(LM.bad_streams(np.concatenate(got, axis=1), st, *LM.expect(channels, true_peak))), t0)


def domain(channels):
    """tests/float_domain_lib.py's streams (NaN, infinities, +-FLT_MAX, overflowing and subnormal samples at 3072 .. 4095) side by
    side, 6000 samples each, under its six (gain, ceiling) pairs (one run per ceiling, a gain per stream), both detectors, one
    call and three: samples (a NaN against a NaN) and statistics against the restatement of each stream alone"""
    import float_domain_lib as FD
    for ceiling in FD.LIMITER_CEILINGS:
        for true_peak in (False, True):
            want = FD.limiter_expect(channels, true_peak, ceiling)
            for cuts in ((FD.LIMITER_T,), FD.LIMITER_CUTS):
                t0 = time.time()
                bad = FD.limiter_bad(FD.limiter_run(EMU, channels, true_peak, ceiling, cuts=cuts), want, channels, ceiling)
                report(f"limiter domain ch{channels} c={float(ceiling):g} tp{true_peak} cuts {list(cuts)} {bad}", len(bad), t0)


CASES = {"parity:1:0": parity, "parity:1:1": parity, "parity:2:0": parity, "parity:2:1": parity, "edges": edges,
         "domain:1": domain, "domain:2": domain}

if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    unknown = [n for n in names if n not in CASES]
    if unknown or not names:
        sys.exit(f"usage: run_emu_limiter.py [--nobuild] CASE ...; cases: {' '.join(CASES)}")
    if "--nobuild" not in sys.argv:
        run_emu.build(strict=True)
    os.environ.setdefault("EMU_STRICT", "1")
    for n in names:
        t = time.time()
        CASES[n](*(int(a) for a in n.split(":")[1:]))
        print(f"{n} done ({time.time() - t:.1f}s)", flush=True)
