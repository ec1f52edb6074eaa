#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the ATRAC3plus frame writer kernel through the CPU SIMT emulator against the oracle."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
from at3_testlib import at3p_specs, at3p_write_frames, at3p_signal
from atracdenc_amd.binding import At3pHip
import run_emu

def domain():
    # tests/float_domain_lib.py's streams through at3phip_encode_frames, whole and as 2 + 1 + 3 frames, against the oracle's PQF -> MDCT -> writer
    import float_domain_lib as FD
    for nch in (2, 1):
        exp = FD.at3p_expect(nch)
        clean = exp[FD.NAMES.index("clean")]
        for split in (None, FD.AT3P_SPLIT):
            t = time.time()
            bad = FD.rows_bad(FD.at3p_run(run_emu.EMU, nch, split=split), exp, "at3p", FD.NAMES, clean)
            print(f"domain nch={nch} split={split}: mismatching frames {len(bad)} {bad} ({time.time()-t:.1f}s)", flush=True)

if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build()
    if "domain" in sys.argv:
        domain()
        sys.exit(0)
    nf = 4
    rng = np.random.RandomState(4)
    for nch in (2, 1):
        cases = [("mix", at3p_specs("mix", nf, nch)), ("burst", at3p_specs("burst", nf, nch)), ("tones", at3p_specs("tones", nf, nch)),
                 ("silence", np.zeros((nf, nch, 2048), np.float32)), ("rand1", (rng.standard_normal((nf, nch, 2048))).astype(np.float32)),
                 ("rand.05", (0.05 * rng.standard_normal((nf, nch, 2048))).astype(np.float32))]
        for name, sp in cases:
            flags = rng.randint(0, 65536, size=(nf, nch)).astype(np.uint16)
            flags[0] = 0; flags[1] = 0xffff; flags[2, 0] = 0x01ff
            for fl in (None, flags):
                t = time.time()
                enc = At3pHip(n_streams=2, max_frames=nf, channels=nch, lib_path=run_emu.EMU)
                got = enc.write_frames(np.stack([sp, sp[::-1]]), None if fl is None else np.stack([fl, fl[::-1]]))
                enc.close()
                exp = np.stack([at3p_write_frames(sp, fl), at3p_write_frames(sp[::-1], None if fl is None else fl[::-1])])
                bad = (got != exp).any(axis=2)
                print(f"nch={nch} {name:8s} flags={'none' if fl is None else 'rand'}: mismatching frames {int(bad.sum())}/{bad.size} ({time.time()-t:.1f}s)", flush=True)
    # PCM to frames
    for nch in (2, 1):
        pcm = np.stack([np.stack([at3p_signal(n, nf, channel=c) for c in range(nch)], axis=-1) for n in ("mix", "burst")])
        enc = At3pHip(n_streams=2, max_frames=nf, channels=nch, lib_path=run_emu.EMU)
        got = np.concatenate([enc.encode_frames(pcm[:, :1]), enc.encode_frames(pcm[:, 1:])], axis=1)
        enc.close()
        exp = np.stack([at3p_write_frames(at3p_specs(n, nf, nch)) for n in ("mix", "burst")])
        print(f"encode nch={nch}: mismatching frames {int((got != exp).any(axis=2).sum())}/{got.shape[0] * got.shape[1]}")
