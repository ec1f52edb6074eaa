#!/usr/bin/env python3
"""The 16-bit instantiations of the kernels that first touch PCM (k_at1_front / k_at1_state, k_at3p_pqf / k_at3p_pqf_state,
k_resample, k_hops / k_carry / k_true_peak / k_scale) through the CPU SIMT harness (tools/emu), against the float instantiations
of the same harness on the widened input ((float)s * 0x1p-15f). Driver of tests/test_s16_simt_harness.py, which runs it in child
processes because the harness reads EMU_STRICT, EMU_FENCE and EMU_ORDER when the library loads.

    run_emu_s16.py [--nobuild] CASE ...

prints one `<what>: bad N` line per comparison (0 is a pass). Every engine runs through the public binding classes with
lib_path= the harness; caller-owned device buffers hold exactly the input (under EMU_FENCE they end or begin at a guard page, so
a 32-bit load that reaches past a row of odd length, or before a row that is only 2-byte aligned, is a fault). CASES lists the
cases."""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import run_emu
import s16_lib as S
from run_emu_decode import DevBuf, report
from atracdenc_amd.binding import (AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, AT3HIP_RESAMPLE_OUT_S16, At1Hip, At3pHip, HipLoudness,
                                   HipResampler)

EMU = run_emu.EMU
HOP = 4410
DEV = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE


def at1(channels):
    """2 streams x 2 blocks, then 1 block of the other kind (the carried block is float for both); host memory, then a device
    buffer of exact size, then one that starts a single sample frame into its allocation (mono: 2-byte aligned)"""
    t0 = time.time()
    p16 = S.pcm16(2, 3 * 512, channels, seed=3 + channels, quiet=(300, 700)).reshape(2, 3, 512, channels)
    pf = S.widen(p16)
    a = At1Hip(n_streams=2, max_blocks=2, channels=channels, lib_path=EMU)
    b = At1Hip(n_streams=2, max_blocks=2, channels=channels, lib_path=EMU)
    want = [b.encode(pf[:, :2]), b.encode(pf[:, 2:])]
    got = [a.encode_s16(p16[:, :2]), a.encode(pf[:, 2:])]
    report(f"at1 ch{channels} s16 then float, host", sum(not S.same_bits(g, w) for g, w in zip(got, want)), t0)
    a.reset()
    got = [a.encode(pf[:, :2]), a.encode_s16(p16[:, 2:])]
    report(f"at1 ch{channels} float then s16, host", sum(not S.same_bits(g, w) for g, w in zip(got, want)))
    a.reset()
    bad = 0
    for off, piece, w in ((0, p16[:, :2], want[0]), (1, p16[:, 2:], want[1])):   # off: sample frames in front of the PCM
        piece = np.ascontiguousarray(piece)
        src, dst = DevBuf(piece.nbytes + 2 * channels * off), DevBuf(w.nbytes)
        ctypes.memmove(src.ptr + 2 * channels * off, piece.ctypes.data, piece.nbytes)
        a.encode_device_s16(src.ptr + 2 * channels * off, piece.shape[1], dst.ptr)
        bad += int(not S.same_bits(dst.read(np.uint8, w.shape), w))
        src.free()
        dst.free()
    report(f"at1 ch{channels} s16 device buffers, one offset by a sample frame", bad)
    a.close()
    b.close()


def at3p(channels):
    """1 stream x 2 frames, then 1 frame of the other kind; host memory and an exact device buffer offset by a sample frame"""
    t0 = time.time()
    p16 = S.pcm16(1, 3 * 2048, channels, seed=20 + channels, quiet=(2500, 3000)).reshape(1, 3, 2048, channels)
    pf = S.widen(p16)
    a = At3pHip(n_streams=1, max_frames=2, channels=channels, lib_path=EMU)
    b = At3pHip(n_streams=1, max_frames=2, channels=channels, lib_path=EMU)
    want = [b.encode_frames(pf[:, :2]), b.encode_frames(pf[:, 2:])]
    got = [a.encode_frames_s16(p16[:, :2]), a.encode_frames(pf[:, 2:])]
    report(f"at3p ch{channels} s16 then float, host", sum(not S.same_bits(g, w) for g, w in zip(got, want)), t0)
    a.reset()
    piece = np.ascontiguousarray(p16[:, 2:])
    src, dst = DevBuf(piece.nbytes + 2 * channels), DevBuf(want[1].nbytes)
    ctypes.memmove(src.ptr + 2 * channels, piece.ctypes.data, piece.nbytes)
    got0 = a.encode_frames(pf[:, :2])
    a.encode_frames_device_s16(src.ptr + 2 * channels, 1, dst.ptr)
    report(f"at3p ch{channels} float then s16 device buffer offset by a sample frame",
           int(not S.same_bits(got0, want[0])) + int(not S.same_bits(dst.read(np.uint8, want[1].shape), want[1])))
    src.free()
    dst.free()
    a.close()
    b.close()


def resample(channels):
    """48000 -> 44100, 3 streams, 300 samples as 199 + 101 (odd: the second mono row is 2-byte aligned) and the flush; float and
    16-bit outputs, exact device buffers"""
    t0 = time.time()
    p16 = S.pcm16(3, 300, channels, seed=40 + channels)
    p16[1] = S.square16(300, channels)
    pf = S.widen(p16)
    a = HipResampler(48000, 44100, channels=channels, n_streams=3, max_in=199, lib_path=EMU)
    b = HipResampler(48000, 44100, channels=channels, n_streams=3, max_in=199, lib_path=EMU)
    want = [b.process(pf[:, :199]), b.process(pf[:, 199:]), b.flush()]
    got = [a.process_s16(p16[:, :199]), a.process(pf[:, 199:]), a.flush()]
    report(f"resample ch{channels} s16 then float, host", sum(not S.same_bits(g, w) for g, w in zip(got, want)), t0)
    got = [a.process(pf[:, :199], out_s16=True), a.process_s16(p16[:, 199:], out_s16=True), a.flush(out_s16=True)]
    report(f"resample ch{channels} 16-bit output", sum(not S.same_bits(g, S.out_s16_of(w)) for g, w in zip(got, want)))
    bad = 0
    for lo, hi, w in ((0, 199, want[0]), (199, 300, want[1])):
        piece = np.ascontiguousarray(p16[:, lo:hi])
        src, dst = DevBuf(piece.nbytes), DevBuf(max(2, S.out_s16_of(w).nbytes))
        n = a.process_s16_ptr(src.write(piece).ptr, hi - lo, dst.ptr, DEV | AT3HIP_RESAMPLE_OUT_S16)
        bad += int(n != w.shape[1] or not S.same_bits(dst.read(np.int16, w.shape), S.out_s16_of(w)))
        src.free()
        dst.free()
    a.reset()
    report(f"resample ch{channels} s16 in and out, exact device buffers", bad)
    a.close()
    b.close()


def loudness(channels):
    """2 streams, 2 hops + 7 samples as 4411 + 4416 (the first odd: the second mono row is 2-byte aligned), true peak on; then
    apply_s16 in its vector and scalar forms"""
    t0 = time.time()
    T = 2 * HOP + 7
    p16 = S.pcm16(2, T, channels, seed=60 + channels, quiet=(5000, 6000))
    pf = S.widen(p16)
    a = HipLoudness(channels=channels, n_streams=2, max_in=HOP + 6, max_hops=2, true_peak=True, lib_path=EMU)
    b = HipLoudness(channels=channels, n_streams=2, max_in=HOP + 6, max_hops=2, true_peak=True, lib_path=EMU)
    b.process(pf[:, :HOP + 1])
    b.process(pf[:, HOP + 1:])
    want_z, want = b.hops(), b.finish()
    a.process_s16(p16[:, :HOP + 1])
    a.process(pf[:, HOP + 1:])
    z, res = a.hops(), a.finish()
    report(f"loudness ch{channels} s16 then float z", int(not S.same_bits(z, want_z)), t0)
    report(f"loudness ch{channels} s16 then float results", sum(bool(S.result_mismatches(x, y)) for x, y in zip(res, want)))
    piece = np.ascontiguousarray(p16[:, :HOP + 1])
    src = DevBuf(piece.nbytes).write(piece)
    a.process_s16_ptr(src.ptr, HOP + 1, AT3HIP_PCM_ON_DEVICE)
    src.free()
    a.process_s16(p16[:, HOP + 1:])
    z, res = a.hops(), a.finish()
    report(f"loudness ch{channels} s16 exact device buffer then s16 host z", int(not S.same_bits(z, want_z)))
    report(f"loudness ch{channels} s16 exact device buffer then s16 host results", sum(bool(S.result_mismatches(x, y)) for x, y in zip(res, want)))
    g = np.array([0.7371, 1.913], np.float32)
    bad = 0
    for n in (1000, 333):
        bad += int(not S.same_bits(a.apply_s16(p16[:, :n], g), b.apply(pf[:, :n], g)))
        piece = np.ascontiguousarray(p16[:, :n])
        src, dst = DevBuf(piece.nbytes).write(piece), DevBuf(2 * piece.nbytes)
        a.apply_s16_ptr(src.ptr, n, g, dst.ptr, DEV)
        bad += int(not S.same_bits(dst.read(np.float32, piece.shape), pf[:, :n] * g[:, None, None]))
        src.free()
        dst.free()
    report(f"loudness ch{channels} apply_s16", bad)
    a.close()
    b.close()


CASES = {"at1:1": at1, "at1:2": at1, "at3p:1": at3p, "at3p:2": at3p, "resample:1": resample, "resample:2": resample,
         "loudness:1": loudness, "loudness:2": loudness}

if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    unknown = [n for n in names if n not in CASES]
    if unknown or not names:
        sys.exit(f"usage: run_emu_s16.py [--nobuild] CASE ...; cases: {' '.join(CASES)}")
    if "--nobuild" not in sys.argv:
        run_emu.build(strict=True)
    os.environ.setdefault("EMU_STRICT", "1")
    for n in names:
        t = time.time()
        CASES[n](*(int(a) for a in n.split(":")[1:]))
        print(f"{n} done ({time.time() - t:.1f}s)", flush=True)
