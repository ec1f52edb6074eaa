#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the ATRAC1 kernels through the CPU SIMT emulator (tools/emu) against the oracle."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
from at3_testlib import SIGNALS, AT1_MODES, at1_blocks, at1_oracle_encode, pcm_stress
from atracdenc_amd.binding import At1Hip
import run_emu

def domain():
    # tests/float_domain_lib.py's streams (NaN, infinities, +-FLT_MAX, overflowing and subnormal samples), one stream per pattern side by
    # side, whole and as 10 + 2 + 12 blocks: sound units and the loudness tap against the oracle's encode of each stream alone
    import float_domain_lib as FD
    for mode, nch in FD.AT1_CASES:
        exp, eloud = FD.at1_expect(mode, nch)
        clean = exp[FD.NAMES.index("clean")]
        for split in (None, FD.AT1_SPLIT):
            t = time.time()
            got, loud = FD.at1_run(run_emu.EMU, mode, nch, split=split)
            bad = FD.rows_bad(got, exp, "at1", FD.NAMES, clean)
            lbad = [n for i, n in enumerate(FD.NAMES) if ("at1", n) not in FD.EXCEPTIONS and FD.floats_match(loud[i], eloud[i]).any()]
            print(f"domain  nch={nch} {mode:10s} split={split}: frames bad {len(bad)} {bad} loud bad {len(lbad)} {lbad} ({time.time()-t:.1f}s)", flush=True)

if __name__ == "__main__":
    if "--nobuild" not in sys.argv: run_emu.build()
    if "domain" in sys.argv:
        domain()
        sys.exit(0)
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["mix", "burst", "stress"]
    gens = dict(SIGNALS); gens["stress"] = pcm_stress
    nb = 6
    for name in names:
        for nch in (2, 1):
            for mode in ("auto", "short", "mask5", "auto_bfu3"):
                auto, mask, bfu = AT1_MODES[mode]
                pcm = np.stack([at1_blocks(gens[name](34 if name == "stress" else nb // 2 + 1), nch)[:nb],
                                at1_blocks(SIGNALS["mix"](nb // 2 + 1, seed=3), nch)[:nb]])
                t = time.time()
                enc = At1Hip(n_streams=2, max_blocks=nb, channels=nch, window_auto=auto, window_mask=mask, bfu_idx_const=bfu,
                             lib_path=run_emu.EMU)
                got = np.concatenate([enc.encode(pcm[:, :4]), enc.encode(pcm[:, 4:])], axis=1)
                specs = enc.read_tap(At1Hip.TAP_SPECTRA, np.float32, (2, nb - 4, nch, 512))
                masks = enc.read_tap(At1Hip.TAP_MASKS, np.int32, (2, nb - 4, nch))
                loud = enc.read_tap(At1Hip.TAP_LOUDNESS, np.float32, (2, nb - 4))
                enc.close()
                exp = [at1_oracle_encode(pcm[i], mode, taps=True) for i in range(2)]
                ef = np.stack([e[0] for e in exp])
                bad = (got != ef).any(axis=3)
                es = np.stack([e[1][4:] for e in exp]); em = np.stack([e[2][4:] for e in exp]); el = np.stack([e[3][4:] for e in exp])
                print(f"{name:7s} nch={nch} {mode:10s}: frames bad {int(bad.sum())}/{bad.size} {np.argwhere(bad)[:4].tolist()} "
                      f"specs bad {int((specs.view(np.uint32) != es.view(np.uint32)).sum())} masks bad {int((masks != em).sum())} "
                      f"loud bad {int((loud.view(np.uint32) != el.view(np.uint32)).sum())} ({time.time()-t:.1f}s)")
