#!/usr/bin/env python3
"""The decoders (ATRAC1, ATRAC3, ATRAC3plus with and without tonal blocks) and the sample-rate converter through the CPU SIMT
harness (tools/emu), against the committed goldens and the C restatements under tests/host, and (the `codebook` family) a slice of
the corpora that hold every code of the ATRAC3 and ATRAC3plus tables at every bit phase. Driver of
tests/test_decoders_simt_harness.py, which runs it in child processes because the harness reads EMU_STRICT, EMU_FENCE and
EMU_ORDER when the library loads.

    run_emu_decode.py [--nobuild] CASE ...

prints one `<what>: bad N` line per comparison (N = mismatching frames, outputs or counters; 0 is a pass). Every engine runs
through the public binding classes with lib_path= the harness. CASES lists the cases."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import run_emu
import at1_decode_lib as A1
import at3_decode_lib as A3
import at3p_decode_lib as AP
import at3p_tonal_lib as AT
import resample_lib as RS
from at3_testlib import pin_digest
from atracdenc_amd.binding import (AT3HIP_OUT_ON_DEVICE, AT3HIP_PCM_ON_DEVICE, AT3PHIP_DECODE_TONES, At1HipDecoder, At3HipDecoder,
                                   At3pHipDecoder, HipResampler)

EMU = run_emu.EMU


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def s16_of(pcm):
    """the decoders' float -> 16-bit rule: lrintf(x * 32767.0f)"""
    return np.rint(pcm.astype(np.float32) * np.float32(32767.0)).astype(np.int16)


def report(what, bad, t0=None):
    print(f"{what}: bad {int(bad)}" + (f" ({time.time() - t0:.1f}s)" if t0 else ""), flush=True)


def frames_bad(got, exp):
    """mismatching frames of [S][N]... arrays, by bit pattern"""
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return got.size + 1
    a = got.view(np.uint32) if got.dtype == np.float32 else got
    b = exp.view(np.uint32) if exp.dtype == np.float32 else exp
    return int((a != b).reshape(got.shape[0], got.shape[1], -1).any(axis=2).sum())


class DevBuf:
    """A caller's device buffer of exactly n bytes from the harness's hipMalloc: under EMU_FENCE it ends (begins) at the guard
    page. The product pads its own allocations (at3_host_util.hpp: dev_alloc), so an overread of a frame staged from host
    memory lands in that slack; a buffer the caller hands over with AT3HIP_PCM_ON_DEVICE / AT3HIP_OUT_ON_DEVICE has none."""

    def __init__(self, nbytes):
        import ctypes
        self.lib = ctypes.CDLL(EMU)
        self.lib.emu_device_alloc.restype = ctypes.c_void_p
        self.lib.emu_device_alloc.argtypes = [ctypes.c_size_t]
        self.lib.emu_device_free.argtypes = [ctypes.c_void_p]
        self.nbytes = int(nbytes)
        self.ptr = self.lib.emu_device_alloc(self.nbytes)
        assert self.ptr

    def write(self, a):
        import ctypes
        a = np.ascontiguousarray(a)
        assert a.nbytes == self.nbytes
        ctypes.memmove(self.ptr, a.ctypes.data, a.nbytes)
        return self

    def read(self, dtype, shape):
        import ctypes
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        ctypes.memmove(out.ctypes.data, self.ptr, out.nbytes)
        return out

    def free(self):
        self.lib.emu_device_free(self.ptr)
        self.ptr = None


def decode_exact(dec, frames, out_shape, flags=0):
    """one call of `dec` on caller-owned device buffers that hold exactly the frames and exactly the PCM"""
    src = DevBuf(frames.nbytes).write(frames)
    dst = DevBuf(4 * int(np.prod(out_shape)))
    dec.decode_ptr(src.ptr, frames.shape[1], dst.ptr, AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE | flags)
    out = dst.read(np.float32, out_shape)
    src.free()
    dst.free()
    return out


def check_share(what, accepted, n_frames):
    """A fuzz run that the restatement mostly rejects proves little about the synthesis kernels: by the RESTATEMENT's own
    account at least a quarter of the frames are accepted and at least one is rejected."""
    accepted = int(accepted)
    print(f"{what}: restatement accepts {accepted} of {n_frames} frames", flush=True)
    assert 4 * accepted >= n_frames, (what, accepted, n_frames)
    assert accepted < n_frames, (what, "no frame is rejected")


# ---- ATRAC1 -------------------------------------------------------------------------------------------------------------------
def at1_counts(dec):
    c = dec.counters()
    return [c["bad_block_size"], c["read_past_end"]]


def at1_accepted(units):
    """[S][N][C][212] -> [S][N] bool from the restatement: no unit of the frame is rejected"""
    ok = np.zeros(units.shape[:2], bool)
    for s in range(units.shape[0]):
        d = A1.CpuDecoder(units.shape[2])
        for f in range(units.shape[1]):
            before = int(d.rejected.sum())
            d.decode(units[s, f:f + 1])
            ok[s, f] = int(d.rejected.sum()) == before
    return ok


def at1_goldens():
    g = np.load(A1.GOLDEN)
    for name in g["cases"]:
        t0 = time.time()
        units = g[f"{name}_units"]
        dec = At1HipDecoder(n_streams=1, max_frames=units.shape[0], channels=units.shape[1], lib_path=EMU)
        got = dec.decode(units[None])[0]
        c = at1_counts(dec)
        dec.close()
        bad = int(not np.array_equal(pin_digest(got), g[f"{name}_pcm_sha256"]))
        if f"{name}_pcm" in g.files:
            bad += frames_bad(got[None], g[f"{name}_pcm"][None])
        report(f"at1 golden {name}", bad, t0)
        report(f"at1 golden {name} counters", c != g[f"{name}_rejected"].tolist())


def at1_compare(what, units, check=True):
    t0 = time.time()
    exp, rej = A1.cpu_ref(A1.cpu_lib(), units)
    if check:
        check_share(what, at1_accepted(units).sum(), units.shape[0] * units.shape[1])
    dec = At1HipDecoder(n_streams=units.shape[0], max_frames=units.shape[1], channels=units.shape[2], lib_path=EMU)
    got = dec.decode(units)
    c = at1_counts(dec)
    dec.close()
    report(what, frames_bad(got, exp), t0)
    report(f"{what} counters", c != rej)


def at1_fuzz(nch):
    at1_compare(f"at1 fuzz ch{nch}", A1.fuzz_units(nch, 6, 600, seed=40 + nch))   # the GPU suite's test_fuzz_equals_restatement


def at1_fuzz_large(nch):
    at1_compare(f"at1 large fuzz ch{nch}", A1.fuzz_units(nch, 8 // nch, 500, seed=9000 + nch))


def at1_state():
    """The split patterns of the GPU suite's test_splits_reset_and_counters scaled down from 300 to 120 units for the time
    budget (there [1, 7, 64, 100, 128], [299, 1] and [13] * 23 + [1]; here the same shapes: uneven pieces, all but one unit
    then one, many equal pieces and a short last one), plus one unit per call and reset() mid-stream."""
    t0 = time.time()
    n = 120
    units = A1.fuzz_units(2, 3, n, seed=7)
    exp, rej = A1.cpu_ref(A1.cpu_lib(), units)
    dec = At1HipDecoder(n_streams=3, max_frames=n, channels=2, lib_path=EMU)
    for cuts in ([1, 7, 48, 64], [n - 1, 1], [13] * (n // 13) + [n % 13], [1] * n):
        dec.decode(units[:, 5:9])   # state and counters that reset() must forget
        dec.reset()
        parts, pos = [], 0
        for k in cuts:
            parts.append(dec.decode(units[:, pos:pos + k]))
            pos += k
        assert pos == n
        report(f"at1 splits {cuts[:3]}..", frames_bad(np.concatenate(parts, axis=1), exp), t0)
        c = dec.counters(reset=True)
        report("at1 splits counters", [c["bad_block_size"], c["read_past_end"]] != rej or at1_counts(dec) != [0, 0])
    dec.close()


def at1_s16():
    g = np.load(A1.GOLDEN)
    for name in ("stress_ch2_auto", "crafted_ch1", "mixed_windows_ch2"):
        units = g[f"{name}_units"][None]
        dec = At1HipDecoder(n_streams=1, max_frames=units.shape[1], channels=units.shape[2], lib_path=EMU)
        f32 = dec.decode(units)
        dec.reset()
        got = dec.decode(units, s16=True)
        dec.close()
        report(f"at1 s16 {name}", int(got.dtype != np.int16) + frames_bad(got, s16_of(f32)) +
               int(not np.array_equal(pin_digest(f32[0]), g[f"{name}_pcm_sha256"])))


def at1_single():
    """Every crafted and random unit, one frame per call on a context of max_frames=1, from and into caller-owned device
    buffers of exactly the frame's and the PCM's size (decode_exact): the unit buffer IS the unit, so under EMU_FENCE an
    overread of a single unit meets the guard page. Units that read past their 212 bytes must be among them."""
    t0 = time.time()
    for nch in (1, 2):
        rng = np.random.default_rng(300 + nch)
        units = np.concatenate([A1.crafted_units(nch, 40 + nch), rng.integers(0, 256, (24 // nch, nch, 212), dtype=np.uint8)])[None]
        exp, rej = A1.cpu_ref(A1.cpu_lib(), units)
        assert rej[1] > 0, "no unit reads past the end"
        dec = At1HipDecoder(n_streams=1, max_frames=1, channels=nch, lib_path=EMU)
        got = np.concatenate([decode_exact(dec, units[:, k:k + 1], (1, 1, 512, nch)) for k in range(units.shape[1])], axis=1)
        c = at1_counts(dec)
        dec.close()
        report(f"at1 one unit per call ch{nch} ({units.shape[1]} frames, {rej[1]} read past the end)", frames_bad(got, exp), t0)
        report(f"at1 one unit per call ch{nch} counters", c != rej)


# ---- ATRAC3 -------------------------------------------------------------------------------------------------------------------
def at3_counts(dec):
    c = dec.counters()
    return [c[r] for r in A3.REASONS]


def at3_accepted(frames, fsz, js):
    ok = np.zeros(frames.shape[:2], bool)
    for s in range(frames.shape[0]):
        _, _, fl = A3.cpu_decode(frames[s], fsz, js, fields=True)
        ok[s] = (fl["reason"] == 0).all(axis=1)
    return ok


def at3_goldens():
    g = np.load(A3.GOLDEN)
    for name in g["cases"]:
        t0 = time.time()
        fsz, js = (int(v) for v in g[f"{name}_row"])
        frames = g[f"{name}_frames"]
        dec = At3HipDecoder(n_streams=1, frame_size=fsz, max_frames=frames.shape[0], lib_path=EMU)
        assert dec.joint_stereo == bool(js)
        got = dec.decode(frames[None])[0]
        c = at3_counts(dec)
        dec.close()
        bad = int(not np.array_equal(pin_digest(got), g[f"{name}_pcm_sha256"]))
        if f"{name}_pcm" in g.files:
            bad += frames_bad(got[None], g[f"{name}_pcm"][None])
        report(f"at3 golden {name}", bad, t0)
        report(f"at3 golden {name} counters", c != g[f"{name}_rejected"].tolist())


def at3_compare(what, frames, fsz, js, check=True):
    t0 = time.time()
    exp, rej = A3.cpu_ref(frames, fsz, js)
    if check:
        check_share(what, at3_accepted(frames, fsz, js).sum(), frames.shape[0] * frames.shape[1])
    dec = At3HipDecoder(n_streams=frames.shape[0], frame_size=fsz, max_frames=frames.shape[1], lib_path=EMU)
    got = dec.decode(frames)
    c = at3_counts(dec)
    dec.close()
    report(what, frames_bad(got, exp), t0)
    report(f"{what} counters", c != rej)


def at3_light_stream(g, fsz, n_frames, seed):
    """[1][n_frames][fsz]: encoder frames of the row, one in four with one bit flipped. fuzz_frames draws half of its frames as
    random bytes and a quarter as encoder frames, so by construction about a quarter of its frames pass the restatement (less
    in the joint-stereo rows, where a flipped bit usually breaks a unit: 69 of 288 in row 192 with the GPU suite's seed). One
    such stream next to fuzz_frames' streams lifts every row's case over check_share's quarter."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([g[f"{c}_frames"] for c in g["cases"] if int(g[f"{c}_row"][0]) == fsz and not c.startswith(("crafted", "random"))])
    enc = pool[rng.integers(0, pool.shape[0], n_frames)]
    return np.where((rng.integers(0, 4, n_frames) == 0)[:, None], A3.mutate_frames(enc, rng, n_flips=1), enc)[None]


def at3_fuzz(part):
    g = np.load(A3.GOLDEN)
    for _, fsz, js in A3.ROWS[part::2]:
        # streams 0-2: the GPU suite's test_fuzz_equals_restatement, byte for byte
        frames = np.concatenate([A3.fuzz_frames(g, fsz, 3, 96, seed=fsz), at3_light_stream(g, fsz, 96, seed=100 + fsz)])
        at3_compare(f"at3 fuzz {fsz}", frames, fsz, js)


def at3_fuzz_large(part):
    g = np.load(A3.GOLDEN)
    for _, fsz, js in A3.ROWS[part::2]:
        frames = np.concatenate([A3.fuzz_frames(g, fsz, 6, 192, seed=7000 + fsz), at3_light_stream(g, fsz, 192, seed=7100 + fsz)])
        at3_compare(f"at3 large fuzz {fsz}", frames, fsz, js)


def at3_state():
    t0 = time.time()
    g = np.load(A3.GOLDEN)
    fsz, js, n = 192, True, 120
    frames = A3.fuzz_frames(g, fsz, 2, n, seed=77)
    exp, rej = A3.cpu_ref(frames, fsz, js)
    dec = At3HipDecoder(n_streams=2, frame_size=fsz, max_frames=n, lib_path=EMU)
    rng = np.random.default_rng(5)
    for trial in range(3):
        cuts = np.arange(1, n) if trial == 2 else np.sort(rng.choice(np.arange(1, n), 5, replace=False))   # trial 2: one frame per call
        parts = [dec.decode(np.ascontiguousarray(p)) for p in np.split(frames, cuts, axis=1)]
        report(f"at3 splits trial {trial}", frames_bad(np.concatenate(parts, axis=1), exp), t0)
        report("at3 splits counters", at3_counts(dec) != rej)
        dec.decode(frames[:, 3:7])   # mid-stream: reset() returns to the initial state
        dec.reset()
        report("at3 reset counters", at3_counts(dec) != [0] * len(A3.REASONS))
    report("at3 reset first frame", frames_bad(dec.decode(frames[:, :1]), exp[:, :1]))
    dec.close()


def at3_s16():
    g = np.load(A3.GOLDEN)
    for name in ("crafted_192", "burst_384_ch2", "random_1024"):
        fsz = int(g[f"{name}_row"][0])
        frames = g[f"{name}_frames"][None]
        dec = At3HipDecoder(n_streams=1, frame_size=fsz, max_frames=frames.shape[1], lib_path=EMU)
        f32 = dec.decode(frames)
        dec.reset()
        got = dec.decode(frames, s16=True)
        dec.close()
        report(f"at3 s16 {name}", int(got.dtype != np.int16) + frames_bad(got, s16_of(f32)) +
               int(not np.array_equal(pin_digest(f32[0]), g[f"{name}_pcm_sha256"])))


def at3_single():
    """as at1_single: every crafted frame of every row and random frames, one per call on a context of max_frames=1"""
    t0 = time.time()
    for _, fsz, js in A3.ROWS:
        rng = np.random.default_rng(500 + fsz)
        frames = np.concatenate([A3.crafted_frames(fsz, js, seed=fsz), rng.integers(0, 256, (8, fsz), dtype=np.uint8)])[None]
        exp, rej = A3.cpu_ref(frames, fsz, js)
        past = rej[A3.REASONS.index("read_past_end")]
        assert past > 0, "no unit reads past the end"
        dec = At3HipDecoder(n_streams=1, frame_size=fsz, max_frames=1, lib_path=EMU)
        got = np.concatenate([decode_exact(dec, frames[:, k:k + 1], (1, 1, 1024, 2)) for k in range(frames.shape[1])], axis=1)
        c = at3_counts(dec)
        dec.close()
        report(f"at3 one frame per call {fsz} ({frames.shape[1]} frames, {past} units read past the end)", frames_bad(got, exp), t0)
        report(f"at3 one frame per call {fsz} counters", c != rej)


# ---- ATRAC3plus ---------------------------------------------------------------------------------------------------------------
def at3p_counts(dec):
    c = dec.counters()
    return [c[r] for r in AP.REASONS]


def at3p_load(path):
    g = np.load(path)
    return g, [str(c) for c in g["cases"]]


def at3p_goldens():
    from at3_testlib import at3p_write_frames
    g, names = at3p_load(AP.GOLDEN)
    for nch in (1, 2):
        t0 = time.time()
        cases = [n for n in names if int(g[f"{n}_channels"]) == nch]
        nf = max(g[f"{n}_frames"].shape[0] for n in cases)
        # every case of this channel count side by side as its own stream, padded with silence frames past its end
        frames = np.zeros((len(cases), nf, 2048), np.uint8)
        pad = at3p_write_frames(np.zeros((1, nch, 2048), np.float32))[0]
        for i, n in enumerate(cases):
            fr = g[f"{n}_frames"]
            frames[i, :fr.shape[0]] = fr
            frames[i, fr.shape[0]:] = pad
        dec = At3pHipDecoder(n_streams=len(cases), channels=nch, max_frames=nf, lib_path=EMU)
        pcm = dec.decode(frames)
        c = at3p_counts(dec)
        dec.close()
        want = np.zeros(len(AP.REASONS), np.int64)
        for i, n in enumerate(cases):
            k = g[f"{n}_frames"].shape[0]
            bad = int(not np.array_equal(pin_digest(pcm[i, :k]), g[f"{n}_pcm_sha256"]))
            if f"{n}_pcm" in g:
                bad += frames_bad(pcm[i:i + 1, :k], g[f"{n}_pcm"][None])
            report(f"at3p golden {n}", bad, t0)
            want += g[f"{n}_rejected"]
        report(f"at3p goldens ch{nch} counters", c != want.tolist())


def at3p_tonal_goldens():
    g, names = at3p_load(AT.GOLDEN)
    for nch in (1, 2):
        t0 = time.time()
        cases, frames = AT.side_by_side(g, names, nch)
        dec = At3pHipDecoder(n_streams=len(cases), channels=nch, max_frames=frames.shape[1], lib_path=EMU)
        pcm = dec.decode(frames, tones=True)
        c = at3p_counts(dec)
        dec.reset()
        s16 = dec.decode(frames, s16=True, tones=True)
        dec.close()
        want = np.zeros(len(AP.REASONS), np.int64)
        for i, n in enumerate(cases):
            k = g[f"{n}_frames"].shape[0]
            report(f"at3p tonal golden {n}", int(not np.array_equal(pin_digest(pcm[i, :k]), g[f"{n}_pcm_sha256"])), t0)
            ref = np.clip(np.rint(pcm[i] * np.float32(32767.0)), -32768, 32767).astype(np.int16)
            report(f"at3p tonal golden {n} s16", frames_bad(s16[i:i + 1], ref[None]))
            want += g[f"{n}_rejected"]
        pad = frames.shape[1] * len(cases) - sum(g[f"{n}_frames"].shape[0] for n in cases)   # zero frames: rejected
        want += pad * AT.cpu_tonal_decode(np.zeros((1, 2048), np.uint8), nch)[1]
        report(f"at3p tonal goldens ch{nch} counters", c != want.tolist())


def at3p_compare(what, frames, nch, tones, check=True):
    """tones=False against tests/host/at3p_decode_cpu.c, tones=True against tests/host/at3p_tonal_cpu.c"""
    t0 = time.time()
    exp, total = [], np.zeros(len(AP.REASONS), np.int64)
    for i in range(frames.shape[0]):
        want, rej = AT.cpu_tonal_decode(frames[i], nch) if tones else AP.cpu_decode(frames[i], nch)
        exp.append(want)
        total += rej
    n = frames.shape[0] * frames.shape[1]
    if check:
        check_share(what, n - int(total.sum()), n)   # (one reason per rejected frame)
    dec = At3pHipDecoder(n_streams=frames.shape[0], channels=nch, max_frames=frames.shape[1], lib_path=EMU)
    got = dec.decode(frames, tones=tones)
    c = at3p_counts(dec)
    dec.close()
    report(what, frames_bad(got, np.stack(exp)), t0)
    report(f"{what} counters", c != total.tolist())


def at3p_tonal_fuzz_streams(nch, streams, nf, seed=None):
    """fuzz_tonal_streams' streams (the pool, flips and seed of the GPU suite's test_fuzzed_tonal_frames_equal_restatement by
    default) and one more that cycles through the crafted tonal goldens, rejected frames among them: two bit flips in a
    tonal frame rarely make it invalid (none of the stereo pool's frames is rejected with the GPU suite's seed), and
    check_share wants the rejection path in every case."""
    crafted = np.load(AT.GOLDEN)[f"crafted_{nch}ch_frames"]
    return np.concatenate([AT.fuzz_tonal_streams(nch, streams, nf, seed), crafted[np.arange(nf) % crafted.shape[0]][None]])


def at3p_fuzz(nch):
    g, names = at3p_load(AP.GOLDEN)
    frames = AP.fuzz_streams(g, names, nch)   # the GPU suite's test_fuzz_equals_restatement
    at3p_compare(f"at3p fuzz ch{nch}", frames, nch, tones=False)
    at3p_compare(f"at3p fuzz ch{nch} tones", frames, nch, tones=True)
    at3p_compare(f"at3p tonal fuzz ch{nch}", at3p_tonal_fuzz_streams(nch, 4, 48), nch, tones=True)


def at3p_fuzz_large(nch):
    g, names = at3p_load(AP.GOLDEN)
    frames = AP.fuzz_streams(g, names, nch, seed=8000 + nch, n_streams=32, n_plain=24, n_head=16, n_crafted=8)
    at3p_compare(f"at3p large fuzz ch{nch}", frames, nch, tones=False)
    at3p_compare(f"at3p large tonal fuzz ch{nch}", at3p_tonal_fuzz_streams(nch, 31, 80, seed=8100 + nch), nch, tones=True)


def at3p_state():
    t0 = time.time()
    g, names = at3p_load(AP.GOLDEN)
    frames = np.concatenate([g["sig_mix_2ch_frames"], g["win_alternating_2ch_frames"], g["crafted_2ch_frames"]])[None]
    n = frames.shape[1]
    want, rej = AP.cpu_decode(frames[0], 2)
    dec = At3pHipDecoder(n_streams=1, channels=2, max_frames=n, lib_path=EMU)
    rng = np.random.default_rng(5)
    for trial in range(4):
        dec.decode(frames[:, 2:5])   # mid-stream
        dec.reset()
        report("at3p reset counters", any(at3p_counts(dec)))
        cuts = np.arange(1, n) if trial == 3 else np.sort(rng.choice(np.arange(1, n), 4, replace=False))   # trial 3: one frame per call
        parts = [dec.decode(frames[:, a:b]) for a, b in zip(np.r_[0, cuts], np.r_[cuts, n])]
        report(f"at3p splits trial {trial}", frames_bad(np.concatenate(parts, axis=1), want[None]), t0)
        c = dec.counters(reset=True)
        report("at3p splits counters", [c[r] for r in AP.REASONS] != rej.tolist())
    dec.close()
    # tonal blocks: the three-record carry across every cut, one frame per call, reset between
    g, names = at3p_load(AT.GOLDEN)
    fr = np.concatenate([g["random_2ch_frames"], g["envelopes_2ch_frames"], g["share_mixed_lead1_frames"]])
    n = fr.shape[0]
    want, rej = AT.cpu_tonal_decode(fr, 2)
    dec = At3pHipDecoder(n_streams=1, channels=2, max_frames=n, lib_path=EMU)
    report("at3p tonal whole", frames_bad(dec.decode(fr[None], tones=True), want[None]), t0)
    report("at3p tonal whole counters", at3p_counts(dec) != rej.tolist())
    for cut in range(1, n):
        dec.reset()
        a = dec.decode(fr[None, :cut], tones=True)
        b = dec.decode(fr[None, cut:], tones=True)
        report(f"at3p tonal cut {cut}", frames_bad(np.concatenate([a, b], axis=1), want[None]))
    dec.reset()
    parts = [dec.decode(fr[None, i:i + 1], tones=True) for i in range(n)]
    report("at3p tonal one frame per call", frames_bad(np.concatenate(parts, axis=1), want[None]), t0)
    dec.close()


def at3p_s16():
    g, _ = at3p_load(AP.GOLDEN)
    frames = np.concatenate([g["sig_stress_2ch_frames"], g["crafted_2ch_frames"]])[None]
    dec = At3pHipDecoder(n_streams=1, channels=2, max_frames=frames.shape[1], lib_path=EMU)
    f = dec.decode(frames)
    dec.reset()
    s = dec.decode(frames, s16=True)
    dec.close()
    report("at3p s16", int(s.dtype != np.int16) + frames_bad(s, s16_of(f)))


def at3p_single():
    """as at1_single: every crafted frame, the crafted tonal frames (one ends inside its tonal block), and random frames, one per
    call on a context of max_frames=1, with and without tonal decoding. Frames that read past the 2048 bytes must be among
    them, by the restatement's counters."""
    t0 = time.time()
    k_past = AP.REASONS.index("read_past_end")
    for nch in (1, 2):
        rng = np.random.default_rng(700 + nch)
        crafted, _ = AP.crafted_frames(nch, seed=77 + nch)
        tonal = np.load(AT.GOLDEN)[f"crafted_{nch}ch_frames"]   # with a frame that ends inside its tonal block
        frames = np.concatenate([crafted, tonal, AT.pool(rng, nch, 8), rng.integers(0, 256, (6, 2048), dtype=np.uint8)])[None]
        for tones in (False, True):
            want, rej = AT.cpu_tonal_decode(frames[0], nch) if tones else AP.cpu_decode(frames[0], nch)
            assert rej[k_past] > 0, ("no frame reads past the end", tones, rej)
            dec = At3pHipDecoder(n_streams=1, channels=nch, max_frames=1, lib_path=EMU)
            got = np.concatenate([decode_exact(dec, frames[:, k:k + 1], (1, 1, 2048, nch), AT3PHIP_DECODE_TONES if tones else 0)
                                  for k in range(frames.shape[1])], axis=1)
            c = at3p_counts(dec)
            dec.close()
            what = f"at3p one frame per call ch{nch} tones={int(tones)}"
            report(f"{what} ({frames.shape[1]} frames, {rej[k_past]} read past the end)", frames_bad(got, want[None]), t0)
            report(f"{what} counters", c != rej.tolist())


# ---- every code at every bit phase --------------------------------------------------------------------------------------------
CODEBOOK_SHIFTS = (0, 7, 31)


def at3p_codebook(nch):
    """A slice of tests/at3p_decode_lib.code_corpus: every table's frame, the group-flag frames and the frame that ends on its
    limit at shifts 0, 7 and 31, through the four instantiations of the unpack kernel (plain / sparse parse x 2048 bytes / the
    corpus' own frame size), against the restatement with the same arguments. Every frame is valid: nothing is rejected."""
    import at3p_writer_lib as W
    c = AP.code_corpus(nch)
    for sparse in (False, True):
        for sized in (False, True):
            t0 = time.time()
            fb = c["bytes"] if sized else AP.FRAME
            frames = np.ascontiguousarray(c["frames"][list(CODEBOOK_SHIFTS), :, :fb])
            exp, rej = W.decode_streams(frames, nch, sparse=sparse)
            dec = At3pHipDecoder(n_streams=frames.shape[0], channels=nch, max_frames=frames.shape[1], lib_path=EMU, frame_bytes=fb if sized else None)
            got = dec.decode(frames, sparse=sparse)
            cnt = at3p_counts(dec)
            dec.close()
            what = f"at3p codebook ch{nch} sparse={int(sparse)} bytes={fb} ({frames.shape[0] * frames.shape[1]} frames)"
            report(what, frames_bad(got, exp), t0)
            report(f"{what} counters", any(cnt) or rej.any())


def at3_codebook():
    """the same slice of tests/at3_decode_lib.code_corpus for k_at3d_unpack: every selector's frame at shifts 0, 7 and 31, plain
    units and joint-stereo frames (the second unit byte-reversed)"""
    for js in (False, True):
        t0 = time.time()
        c = A3.code_corpus(js)
        frames = np.ascontiguousarray(c["frames"][list(CODEBOOK_SHIFTS)])
        exp, rej = A3.cpu_ref(frames, c["frame_sz"], js)
        dec = At3HipDecoder(n_streams=frames.shape[0], frame_size=c["frame_sz"], max_frames=frames.shape[1], lib_path=EMU)
        got = dec.decode(frames)
        cnt = at3_counts(dec)
        dec.close()
        report(f"at3 codebook js={int(js)} ({frames.shape[0] * frames.shape[1]} frames)", frames_bad(got, exp), t0)
        report(f"at3 codebook js={int(js)} counters", any(cnt) or any(rej))


# ---- the sample-rate converter ------------------------------------------------------------------------------------------------
def restated(pair, x, channels):
    return RS.CpuResampler(*pair, channels).whole(x)


def resample_pairs(part):
    """all 22 pairs (every other one per part) x {1, 2} channels, the four signal kinds side by side, one call / random cuts,
    flush, reset() mid-stream"""
    kinds = ("noise", "sweep", "silence", "subnormal")
    for pair in RS.PAIRS[part::2]:
        for channels in (1, 2):
            t0 = time.time()
            T = 3 * RS.shape(*pair)[2] + 150   # a few filter lengths: history, input and zeros past the end all take part
            xs = np.stack([RS.signal(k, T, channels, seed=i, rate=pair[0]) for i, k in enumerate(kinds)])
            exp = [restated(pair, xs[i], channels) for i in range(len(kinds))]
            rng = np.random.RandomState(pair[0] + 3 * pair[1] + channels)
            r = HipResampler(*pair, channels=channels, n_streams=len(kinds), max_in=T, lib_path=EMU)
            bad = 0
            for trial in range(2):
                cuts = [T] if trial == 0 else sorted(set(rng.randint(0, T, 5).tolist())) + [T]
                got = RS.run_split(r, xs, cuts)
                bad += sum(not RS.bits_equal(got[i], exp[i]) for i in range(len(kinds)))
            r.process(xs[:, :T // 3])
            r.reset()
            got = RS.run_split(r, xs, [T])
            bad += sum(not RS.bits_equal(got[i], exp[i]) for i in range(len(kinds)))
            r.close()
            report(f"resample {pair[0]}-{pair[1]} ch{channels} T={T}", bad, t0)


def resample_tiles(pair, channels, cuts):
    """[(gridDim.x, n0, n_end)] of the calls ending at `cuts` and of the flush, as resample.hip computes them: Q is
    at3hip_resampler_create's largest tile whose padded span fits 80 KB of LDS, the tile count is launch()'s formula"""
    L, M, K = RS.shape(*pair)
    pad = 1 if M % 2 == 0 else 0
    Q = 64
    while Q > 1:
        span = Q * M + K - 1
        if (span + pad * (span // M) + 1) * channels * 4 <= 80 * 1024:
            break
        Q -= 1
    out, t_out = [], 0
    for a in [c - K // 2 for c in cuts] + [cuts[-1]]:
        n_end = max(t_out, -(-a * L // M) if a > 0 else 0)
        out.append((((n_end - 1) // L - t_out // L) // Q + 1 if n_end > t_out else 1, t_out, n_end))
        t_out = n_end
    return out


def resample_edges():
    # the GPU suite's test_max_out_and_empty_calls: n_in < K, n_in = 0, flush of an empty stream
    t0 = time.time()
    r = HipResampler(44100, 192000, channels=2, n_streams=3, max_in=100, lib_path=EMU)
    L, M, K = RS.shape(44100, 192000)
    bad = int(r.max_out != max(-(-100 * L // M), -(-(K // 2) * L // M)))
    x = RS.signal("noise", 100, 2, 5)
    xs = np.stack([x, x * 0.5, -x])
    bad += int(r.process(xs[:, :0]).shape != (3, 0, 2))
    got = RS.run_split(r, xs, [1, 1, 2, 50, 100])
    for i, s in enumerate((1.0, 0.5, -1.0)):
        bad += int(not RS.bits_equal(got[i], restated((44100, 192000), np.float32(s) * x, 2)))
    bad += int(r.flush().shape != (3, 0, 2))
    r.close()
    report("resample max_in=100, empty calls, empty flush", bad, t0)
    # Many tiles (blockIdx.x > 0). The first two pairs have L = 1, so a tile is Q outputs: both calls launch more than 64
    # tiles. The third has L = 147: its second call begins and ends inside a q, so tile 0 begins before n0 and the last of its
    # several tiles ends after n_end. The counts are asserted with the launch's own formula before comparing.
    for pair, channels, T, want_tiles, mid_q in (((44100, 22050), 2, 20000, 65, False), ((88200, 44100), 1, 30000, 65, False),
                                                 ((48000, 44100), 2, 40000, 3, True)):
        t0 = time.time()
        L, M, K = RS.shape(*pair)
        cuts = [T // 3 + 1, T]
        tiles = resample_tiles(pair, channels, cuts)
        print(f"resample {pair[0]}-{pair[1]} ch{channels}: tiles per call {[t for t, _, _ in tiles]}", flush=True)
        assert max(t for t, _, _ in tiles) >= want_tiles, tiles
        n_tiles, n0, n_end = tiles[1]
        if mid_q:
            assert n_tiles >= want_tiles and n0 % L and n_end % L, tiles[1]
        x = RS.signal("noise", T, channels, seed=11)
        r = HipResampler(*pair, channels=channels, n_streams=1, max_in=T, lib_path=EMU)
        got = RS.run_split(r, x[None], cuts)
        r.close()
        report(f"resample {pair[0]}-{pair[1]} ch{channels} {max(t for t, _, _ in tiles)} tiles", not RS.bits_equal(got[0], restated(pair, x, channels)), t0)
    # caller-owned device buffers of exactly the input's and the outputs' size (as decode_exact: under EMU_FENCE they end or
    # begin at the guard page), three calls and the flush
    t0 = time.time()
    bad = 0
    for pair, channels in (((48000, 44100), 2), ((44100, 96000), 1), ((11025, 44100), 2)):
        L, M, K = RS.shape(*pair)
        T = K + 77
        xs = np.stack([RS.signal("noise", T, channels, seed=70 + i, rate=pair[0]) for i in range(2)])
        r = HipResampler(*pair, channels=channels, n_streams=2, max_in=T, lib_path=EMU)
        parts, at, emitted = [], 0, 0
        for cut in (5, K // 2 + 9, T, None):   # None: the flush
            n_end = RS.n_outputs(at if cut is None else 0, *pair) if cut is None else max(emitted, -(-(cut - K // 2) * L // M) if cut > K // 2 else 0)
            n = n_end - emitted
            dst = DevBuf(max(n, 0) * 2 * channels * 4)
            if cut is None:
                got_n = r.flush_ptr(dst.ptr, AT3HIP_OUT_ON_DEVICE)
            else:
                piece = np.ascontiguousarray(xs[:, at:cut])
                src = DevBuf(piece.nbytes).write(piece)
                got_n = r.process_ptr(src.ptr, cut - at, dst.ptr, AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE)
                src.free()
                at = cut
            bad += int(got_n != n)
            parts.append(dst.read(np.float32, (2, max(n, 0), channels)))
            dst.free()
            emitted = n_end
        r.close()
        got = np.concatenate(parts, axis=1)
        bad += sum(not RS.bits_equal(got[i], restated(pair, xs[i], channels)) for i in range(2))
    report("resample caller-owned exact buffers", bad, t0)
    # more than 8 streams
    t0 = time.time()
    pair, T = (32000, 44100), 700
    xs = np.stack([RS.signal(("noise", "sweep")[i % 2], T, 2, seed=60 + i, rate=32000) for i in range(11)])
    r = HipResampler(*pair, channels=2, n_streams=11, max_in=T, lib_path=EMU)
    got = RS.run_split(r, xs, [3, 350, T])
    r.close()
    report("resample 11 streams", sum(not RS.bits_equal(got[i], restated(pair, xs[i], 2)) for i in range(11)), t0)


def resample_domain():
    """tests/float_domain_lib.py's streams (NaN, infinities, +-FLT_MAX, overflowing and subnormal samples) side by side: both directions between
    48000 and 44100, 1 and 2 channels, float and 16-bit output, one call and three, against the restatement of each stream alone"""
    import float_domain_lib as FD
    for pair in FD.RESAMPLE_PAIRS:
        for channels in (1, 2):
            exp = FD.resample_expect(pair, channels)
            for s16 in (False, True):
                t0 = time.time()
                bad = 0
                for cuts in ((FD.RESAMPLE_T,), FD.RESAMPLE_CUTS):
                    bad += len(FD.resample_bad(FD.resample_run(EMU, pair, channels, s16, cuts=cuts), exp, s16))
                report(f"resample domain {pair[0]}-{pair[1]} ch{channels} s16={int(s16)}", bad, t0)


# cases that take an argument are named case:argument (a channel count, or which half of the rows / pairs: 0 or 1)
CASES = {"at1_goldens": at1_goldens, "at3_goldens": at3_goldens, "at3p_goldens": at3p_goldens, "at3p_tonal_goldens": at3p_tonal_goldens,
         "at1_fuzz:1": at1_fuzz, "at1_fuzz:2": at1_fuzz, "at3_fuzz:0": at3_fuzz, "at3_fuzz:1": at3_fuzz,
         "at3p_fuzz:1": at3p_fuzz, "at3p_fuzz:2": at3p_fuzz,
         "at1_fuzz_large:1": at1_fuzz_large, "at1_fuzz_large:2": at1_fuzz_large, "at3_fuzz_large:0": at3_fuzz_large,
         "at3_fuzz_large:1": at3_fuzz_large, "at3p_fuzz_large:1": at3p_fuzz_large, "at3p_fuzz_large:2": at3p_fuzz_large,
         "at1_state": at1_state, "at3_state": at3_state, "at3p_state": at3p_state,
         "at1_s16": at1_s16, "at3_s16": at3_s16, "at3p_s16": at3p_s16,
         "at1_single": at1_single, "at3_single": at3_single, "at3p_single": at3p_single,
         "resample_pairs:0": resample_pairs, "resample_pairs:1": resample_pairs, "resample_edges": resample_edges,
         "resample_domain": resample_domain, "at3p_codebook:1": at3p_codebook, "at3p_codebook:2": at3p_codebook,
         "at3_codebook": at3_codebook}

if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    unknown = [n for n in names if n not in CASES]
    if unknown or not names:
        sys.exit(f"usage: run_emu_decode.py [--nobuild] CASE ...; cases: {' '.join(CASES)}")
    if "--nobuild" not in sys.argv:
        run_emu.build(strict=True)
    os.environ.setdefault("EMU_STRICT", "1")
    for n in names:
        t = time.time()
        CASES[n](*(int(a) for a in n.split(":")[1:]))
        print(f"{n} done ({time.time() - t:.1f}s)", flush=True)
