#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the ATRAC3plus adaptive writer (k_at3p_write_adaptive, k_at3p_write_adaptive_tonal) and the decoder's
kernels at frame sizes other than 2048 bytes through the CPU SIMT emulator, against the restatement tests/host/at3p_writer_cpu.c.
Driver of tests/test_at3p_rate_cpu.py, which runs it in child processes because the harness reads EMU_STRICT, EMU_FENCE, EMU_ORDER
and EMU_STREAMS when the library loads.

    run_emu_at3p_rate.py [--nobuild] [CASE ...]      CASE: signals, tonal, odd, queued (default: all but queued)

Every buffer a kernel reads frames from or writes frames to is a caller's device buffer of exactly [S][F][frame_bytes] bytes
(DevBuf): under EMU_FENCE it ends or begins at a guard page, so a store or a load that still assumes 2048 bytes per frame faults.
Prints one `<what>: bad N` line per comparison (0 is a pass)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import at3p_writer_lib as W
import at3p_tonal_write_lib as TW
from atracdenc_amd.binding import (AT3HIP_ASYNC, AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, AT3PHIP_ALLOC_ADAPTIVE, AT3PHIP_DECODE_TONES,
                                   AT3PHIP_TONES_GATED, AT3PHIP_TONES_SHARED, At3pHip, At3pHipDecoder, pack_tonal_blocks)
import run_emu
from run_emu_decode import DevBuf, bits, report

DEV = AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE
SIZES = {1: (W.MIN_BYTES[1], 376, 2040), 2: (W.MIN_BYTES[2], 376, 2040)}


def write_exact(enc, specs, fb, recs=None):
    """at3phip_write_frames(_tonal) with the flag, spectra and frames in device buffers of exactly their size"""
    S, F = specs.shape[:2]
    src, dst = DevBuf(specs.nbytes).write(specs), DevBuf(S * F * fb)
    if recs is None:
        enc.write_frames_ptr(src.ptr, F, None, dst.ptr, DEV | AT3PHIP_ALLOC_ADAPTIVE)
    else:
        enc.write_frames_tonal_ptr(src.ptr, F, None, recs.ctypes.data, dst.ptr, DEV | AT3PHIP_ALLOC_ADAPTIVE)
    out = dst.read(np.uint8, (S, F, fb))
    src.free()
    dst.free()
    return out


def decode_exact(dec, frames, tones):
    S, F, fb = frames.shape
    src, dst = DevBuf(frames.nbytes).write(frames), DevBuf(4 * S * F * 2048 * dec.channels)
    dec.decode_ptr(src.ptr, F, dst.ptr, DEV | (AT3PHIP_DECODE_TONES if tones else 0))
    out = dst.read(np.float32, (S, F, 2048, dec.channels))
    src.free()
    dst.free()
    return out


def run(name, nch, fb, specs, blocks=None):
    """specs [S][F][C][2048], blocks [S][F] dicts or None: the writer against the restatement, then the decoder (tones on) on
    the restatement's frames: PCM bit for bit and the rejection counters"""
    t = time.time()
    S, F = specs.shape[:2]
    enc = At3pHip(n_streams=S, max_frames=F, channels=nch, lib_path=run_emu.EMU, frame_bytes=fb)
    recs = None if blocks is None else np.stack([pack_tonal_blocks(row, nch) for row in blocks])
    got = write_exact(enc, specs, fb, recs)
    enc.close()
    exp = np.stack([W.write_adaptive(specs[s], fb, blocks=None if blocks is None else blocks[s]) for s in range(S)])
    report(f"{name} nch={nch} size={fb} writer", (got != exp).any(axis=2).sum())
    dec = At3pHipDecoder(n_streams=S, channels=nch, max_frames=F, lib_path=run_emu.EMU, frame_bytes=fb)
    pcm = decode_exact(dec, exp, True)
    cnt = dec.counters()
    dec.close()
    epcm, erej = W.decode_streams(exp, nch, True)
    report(f"{name} nch={nch} size={fb} decoder", (bits(pcm) != bits(epcm)).reshape(S, F, -1).any(axis=2).sum())
    report(f"{name} nch={nch} size={fb} counters {list(cnt.values())}", list(cnt.values()) != erej.tolist(), t)


def queued(nch, fb=376):
    """Calls that are only queued, each followed by the setter - whose wait is what makes the change legal while the call is in
    flight - and by a queued call at fb, all against the restatement:
      at3phip_encode_frames (k_at3p_write_adaptive) at 2048, at3phip_set_frame_bytes(fb), the same call at fb;
      at3phip_encode_frames_tonal with gates and sharing (the tone analysis, k_at3p_write_adaptive_tonal) likewise;
      at3phip_decode with tones (k_at3pd_unpack, k_at3pd_synth, k_at3pd_state) at 2048, at3phip_decoder_set_frame_bytes(fb), then
      at fb (k_at3pd_unpack_sized) on the same stream, whose state carries over the change."""
    import at3p_gha_lib as G
    from at3_testlib import at3p_signal
    F = 3
    ASY = DEV | AT3HIP_ASYNC | AT3PHIP_ALLOC_ADAPTIVE

    def two_calls(raw, x, flags):
        """x [1][2 F][2048][C]: (frames of the first call at 2048, of the second at fb)"""
        enc = At3pHip(n_streams=1, max_frames=F, channels=nch, lib_path=run_emu.EMU)
        src = [DevBuf(x[:, :F].nbytes).write(x[:, :F]), DevBuf(x[:, F:].nbytes).write(x[:, F:])]
        dst = [DevBuf(F * 2048), DevBuf(F * fb)]
        raw(enc)(src[0].ptr, F, dst[0].ptr, flags)
        enc.set_frame_bytes(fb)
        raw(enc)(src[1].ptr, F, dst[1].ptr, flags)
        enc.sync()
        got = [dst[0].read(np.uint8, (F, 2048)), dst[1].read(np.uint8, (F, fb))]
        enc.close()
        for b in src + dst:
            b.free()
        return got

    t = time.time()
    x = np.stack([at3p_signal("mix", 2 * F, channel=c) for c in range(nch)], axis=-1)[None].astype(np.float32)
    got = two_calls(lambda e: e.encode_frames_ptr, x, ASY)
    sp = W.specs_of("mix", nch, 2 * F)
    report(f"queued nch={nch} encode, first call at 2048", (got[0] != W.write_adaptive(sp[:F], 2048)).any(axis=1).sum())
    report(f"queued nch={nch} encode, second call at {fb}", (got[1] != W.write_adaptive(sp[F:], fb)).any(axis=1).sum(), t)

    t = time.time()
    xt = (G.twin_pcm("tones", 2 * F) if nch == 2 else G.signal_pcm("tones", 2 * F, 1))[None].astype(np.float32)
    got = two_calls(lambda e: e.encode_frames_tonal_ptr, xt, ASY | AT3PHIP_TONES_GATED | AT3PHIP_TONES_SHARED)
    kept = {}

    def grab(specs, recs):
        kept["specs"], kept["recs"] = specs, recs
        return np.zeros((specs.shape[0], 2048), np.uint8)
    _, blocks, _ = G.pipeline(xt[0], True, True, grab)
    assert sum(G.n_waves(b) for b in blocks[:-1]) > 0
    exp = [W.write_adaptive(kept["specs"][:F], 2048, blocks=kept["recs"][:F]), W.write_adaptive(kept["specs"][F:], fb, blocks=kept["recs"][F:])]
    report(f"queued nch={nch} tonal encode, first call at 2048", (got[0] != exp[0]).any(axis=1).sum())
    report(f"queued nch={nch} tonal encode, second call at {fb}", (got[1] != exp[1]).any(axis=1).sum(), t)

    t = time.time()   # the decoder on those tonal frames: one stream, three frames of 2048 bytes, then three of fb
    dec = At3pHipDecoder(n_streams=1, channels=nch, max_frames=F, lib_path=run_emu.EMU)
    src = [DevBuf(exp[0].nbytes).write(exp[0]), DevBuf(exp[1].nbytes).write(exp[1])]
    dst = [DevBuf(4 * F * 2048 * nch), DevBuf(4 * F * 2048 * nch)]
    dec.decode_ptr(src[0].ptr, F, dst[0].ptr, DEV | AT3HIP_ASYNC | AT3PHIP_DECODE_TONES)
    dec.set_frame_bytes(fb)
    dec.decode_ptr(src[1].ptr, F, dst[1].ptr, DEV | AT3HIP_ASYNC | AT3PHIP_DECODE_TONES)
    dec.sync()
    pcm = [d.read(np.float32, (F, 2048, nch)) for d in dst]
    cnt = dec.counters()
    dec.close()
    for b in src + dst:
        b.free()
    ref = W.Decoder(nch, True)
    want = [ref.decode(exp[0]), ref.decode(exp[1])]
    report(f"queued nch={nch} decode, first call at 2048", (bits(pcm[0]) != bits(want[0])).reshape(F, -1).any(axis=1).sum())
    report(f"queued nch={nch} decode, second call at {fb}", (bits(pcm[1]) != bits(want[1])).reshape(F, -1).any(axis=1).sum())
    report(f"queued nch={nch} decode, counters {list(cnt.values())}", list(cnt.values()) != ref.rejected.astype(np.int64).tolist(), t)


if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build("--strict" in sys.argv)
    want = [a for a in sys.argv[1:] if not a.startswith("--")]
    for nch in (2, 1):
        for fb in SIZES[nch]:
            if not want or "signals" in want:    # a loud signal and silence beside full-scale noise
                run("signals", nch, fb, np.stack([np.concatenate([W.specs_of("mix", nch, 1), W.specs_of("silence", nch, 1)]),
                                                  W.full_scale_noise(2, nch)]))
            if not want or "tonal" in want:      # the largest record on a full-scale frame and on silence, beside no record and a small one
                sp = np.stack([np.concatenate([W.full_scale_noise(1, nch, seed=4), np.zeros((1, nch, 2048), np.float32)]), W.specs_of("mix", nch, 2)])
                run("tonal", nch, fb, sp, [[TW.largest_block(nch), TW.largest_block(nch)], [None, TW.case_blocks(f"small_{nch}")[0][0]]])
            if not want or "odd" in want:
                run("odd", nch, fb, np.stack([W.odd_specs(nch, 2), W.specs_of("noise", nch, 2)]))
        if "queued" in want:
            queued(nch)
