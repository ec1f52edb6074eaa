"""The adaptive and sparse ATRAC3plus writer kernels (csrc/at3p_alloc.hip, csrc/at3p_sparse.hip) against frames the REFERENCE's part
coders wrote: tests/golden/at3p_ref_parts.npz (tools/gen_golden_at3p_ref_parts.py), with no restatement in between. Per cell -
mono at 176, 376 and 2048 bytes, stereo at 224, 376 and 2048, and one cell with tonal blocks and window flags per channel count,
each with AT3PHIP_ALLOC_ADAPTIVE and again with AT3PHIP_ALLOC_SPARSE added - at3phip_write_frames (at3phip_write_frames_tonal for
the tonal cells) writes 3 streams x 4 frames once from host buffers as a waiting call and once from device buffers as a queued
call. The inputs come from the seeded builders; their hash is checked against the file's before they are used."""
import numpy as np
import pytest

import at3p_ref_parts_lib as P

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def B():
    from atracdenc_amd import binding
    return binding


@pytest.mark.parametrize("cell", P.cells(), ids=lambda c: c[0])
def test_kernels_write_the_references_frames(B, cell):
    import torch
    key, nch, fb, sparse, tonal = cell
    g, meta = P.golden_load()
    specs, flags, blocks, sha = P.cell_inputs(nch, tonal)
    assert meta[key]["inputs_sha256"] == sha and (meta[key]["frame_bytes"], meta[key]["sparse"]) == (fb, sparse)
    want = g[f"{key}_frames"]
    assert want.shape == (P.G_S, P.G_F, fb)
    recs = np.stack([B.pack_tonal_blocks(row, nch) for row in blocks]) if tonal else None
    alloc = B.AT3PHIP_ALLOC_ADAPTIVE | (B.AT3PHIP_ALLOC_SPARSE if sparse else 0)
    n = P.G_S * P.G_F * fb
    enc = B.At3pHip(n_streams=P.G_S, max_frames=P.G_F, channels=nch)
    try:
        enc.set_frame_bytes(fb)
        assert enc.frame_bytes == fb
        waiting = enc.write_frames(specs, flags, recs, adaptive=True, sparse=sparse)
        d_specs = torch.from_numpy(specs).cuda()
        d_out = torch.full((n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dev = B.AT3HIP_PCM_ON_DEVICE | B.AT3HIP_OUT_ON_DEVICE | B.AT3HIP_ASYNC | alloc
        if tonal:
            enc.write_frames_tonal_ptr(d_specs.data_ptr(), P.G_F, flags.ctypes.data, recs.ctypes.data, d_out.data_ptr(), dev)
        else:
            enc.write_frames_ptr(d_specs.data_ptr(), P.G_F, None, d_out.data_ptr(), dev)
        enc.sync()
        queued = d_out.cpu().numpy()
    finally:
        enc.close()
    bad = [(s, f) for s in range(P.G_S) for f in range(P.G_F) if not np.array_equal(waiting[s, f], want[s, f])]
    assert bad == [], f"waiting call: frames {bad} differ from the reference's"
    assert (queued[n:] == SENTINEL).all()
    assert np.array_equal(queued[:n].reshape(P.G_S, P.G_F, fb), want)
