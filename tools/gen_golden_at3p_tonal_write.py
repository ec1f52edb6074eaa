#!/usr/bin/env python3
"""Write tests/golden/at3p_tonal_write.npz: what at3phip_write_frames_tonal and the C++ mirror's analysed schedule must give.

Writer cases (tests/at3p_tonal_write_lib.py, WRITER_CASES): per case 2 streams x 3 frames of white spectra - stored as their
seed - with blocks stored as flat ints and, for one case, window flags; the frames are the REFERENCE's
TAt3PBitStream::WriteFrame(channels, &block or nullptr, sces) after its ScaleFrame (ref_write_tonal_win, which is
at3p_tonal_lib.ref_write_tonal with window flags; the generator checks that the two agree where there are none). For the case
"loud" the seed is searched so that the reference keeps fewer quant units with the largest block than without.
Schedule cases: the frames of the REFERENCE's own TAt3PEnc (atrac/at3p/at3p.cpp compiled as it is) for UseGha = 0, 1, 5 and 7,
with MakeGhaProcessor0 defined by the driver as the stand-in analyser of tests/host/at3p_fake_gha.h (a counter-derived block on
two calls of three; one subband of the writable previous buffers halved).
Nothing compiled from the reference is stored. Run where oracle/_ref and the reference sources exist."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import at3p_tonal_lib as T   # noqa: E402
import at3p_tonal_write_lib as L   # noqa: E402


def loud_seed():
    """the first seed whose frames all keep fewer units under the largest block than without a block"""
    cid = "loud_2"
    blocks = L.case_blocks(cid)
    for seed in range(1, 200):
        specs = L.case_specs(cid, seed)
        ok = True
        for s in range(L.STREAMS):
            with_b = L.ref_write_tonal_win(specs[s], blocks[s])
            none = L.ref_write_tonal_win(specs[s], [None] * L.FRAMES)
            for f in range(L.FRAMES):
                if blocks[s][f] is not None and blocks[s][f]["nb"] == 16 and not T.n_qu(with_b[f]) < T.n_qu(none[f]):
                    ok = False
        if ok:
            return seed
    raise SystemExit("no seed shows the difference")


def main():
    assert L.have_ref(), "needs oracle/_ref and the reference sources"
    seed = loud_seed()
    assert seed == L.LOUD_SEED, f"at3p_tonal_write_lib.LOUD_SEED must be {seed}"
    out = {}
    for cid in L.writer_case_ids():
        nch = int(cid.rsplit("_", 1)[1])
        specs, blocks, flags = L.case_specs(cid), L.case_blocks(cid), L.case_flags(cid)
        frames = np.stack([L.ref_write_tonal_win(specs[s], blocks[s], None if flags is None else flags[s]) for s in range(L.STREAMS)])
        if flags is None:
            assert np.array_equal(frames, np.stack([T.ref_write_tonal(specs[s], blocks[s]) for s in range(L.STREAMS)])), cid
        out[f"{cid}_seed"] = np.int64(L.case_seed(cid))
        out[f"{cid}_blocks"] = L.block_ints(nch, blocks)
        out[f"{cid}_frames"] = frames
        if flags is not None:
            out[f"{cid}_flags"] = flags
        print(cid, "units", [[T.n_qu(f) for f in row] for row in frames])
    for nch, use_gha in L.SCHEDULE_CASES:
        fr = L.ref_schedule(nch, use_gha)
        assert fr.shape == (L.SCHEDULE_CALLS - 1, 2048), fr.shape
        out[f"schedule_{nch}_{use_gha}"] = fr
        print("schedule", nch, use_gha, "units", [T.n_qu(f) for f in fr], "tonal frames",
              int(sum(r[0] for r in T.unpack_tonal(fr, nch)[2])))
    np.savez_compressed(L.GOLDEN, **out)
    print("wrote", L.GOLDEN, os.path.getsize(L.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
