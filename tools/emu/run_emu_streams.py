#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: every engine's stream pipeline through the CPU SIMT harness (tools/emu) in its deferred-stream mode
(EMU_STREAMS, hip/hip_runtime.h): queued calls of unequal size, the host-buffer pipeline, callers' streams with a queued producer
over poison, back-to-back calls that share a staging slot. Driver of tests/test_stream_order_simt_harness.py, which runs every
case in child processes under EMU_STREAMS unset, lazy and lazy:SEED (the harness reads it when the library loads).

    run_emu_streams.py [--nobuild] CASE ...

prints one `<what>: bad N` line per comparison (N = mismatching frames, outputs or streams; 0 is a pass), each against the oracle
or the C restatement the engine's other tests use - never against another run of the engine. CASES lists the cases. A missing
or misplaced wait shows as a mismatch in some mode; EMU_STREAMS_LOG=<file> then records the order in which the operations ran."""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import run_emu
from run_emu_decode import frames_bad, report
from atracdenc_amd import binding as b

EMU = run_emu.EMU
DEV = b.AT3HIP_PCM_ON_DEVICE | b.AT3HIP_OUT_ON_DEVICE
ASYNC = b.AT3HIP_ASYNC
at = lambda a: a.ctypes.data


class Caller:
    """a stream the engines did not make, and the caller's own work on it: copies that are deferred like any queued operation"""

    def __init__(self):
        self.lib = ctypes.CDLL(EMU)
        self.lib.emu_caller_stream_create.restype = ctypes.c_void_p
        self.lib.emu_caller_stream_destroy.argtypes = [ctypes.c_void_p]
        self.lib.emu_caller_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        self.lib.emu_caller_stream_sync.argtypes = [ctypes.c_void_p]
        self.handle = self.lib.emu_caller_stream_create()
        self.keep = []

    def copy(self, dst, src):
        """dst[...] = src, queued: both arrays stay alive and untouched until sync()"""
        assert dst.nbytes == src.nbytes and dst.flags.c_contiguous and src.flags.c_contiguous
        self.keep += [dst, src]
        self.lib.emu_caller_copy(at(dst), at(src), src.nbytes, self.handle)

    def sync(self):
        self.lib.emu_caller_stream_sync(self.handle)
        self.keep = []

    def close(self):
        self.lib.emu_caller_stream_destroy(self.handle)


def mode():
    lib = ctypes.CDLL(EMU)
    return ("eager", "lazy", "seeded")[lib.emu_streams_mode()]


# ---- the ATRAC3 encoder: three compute streams and a copy stream --------------------------------------------------------------
AT3_CALLS = (3, 1, 1, 3, 1, 2)
S = 2


def at3_signals(nb):
    from at3_testlib import SIGNALS
    pcm = np.stack([SIGNALS["mix"](nb, seed=31), SIGNALS["burst"](nb, phase=300)])
    p16 = np.round(np.clip(pcm, -1.0, 32767.0 / 32768.0) * 32768.0).astype(np.int16)
    return (p16.astype(np.float32) / np.float32(32768.0)).astype(np.float32), p16   # (the floats are the 16-bit samples)


def at3_expect(pcm, br, ng):
    from at3_testlib import oracle
    return np.stack([oracle().encode(pcm[i], br, ng, 0)[0] for i in range(pcm.shape[0])])


def at3_queued(enc, pcm, decoy=None, timing=False):
    """asynchronous device-pointer calls of AT3_CALLS blocks, each into its own output, one sync(); with `decoy` on a caller's
    stream whose queued copy writes each call's PCM over a buffer that held the decoy signal"""
    if timing:
        enc.set_option(b.OPT_TIMING_EVERY, 1)
    caller = Caller() if decoy is not None else None
    if caller:
        enc.set_stream(caller.handle)
    src = np.ascontiguousarray(decoy if caller else pcm).copy()
    outs, counts, pos = [], [], 0
    for n in AT3_CALLS:
        out = np.full((S, n, enc.frame_size), 0xEE, np.uint8)
        piece = np.ascontiguousarray(src[:, pos:pos + n])   # (a buffer of its own per call: nothing says when a call has read its input)
        if caller:
            caller.copy(piece, np.ascontiguousarray(pcm[:, pos:pos + n]))
        outs.append((out, piece))
        counts.append(enc.encode_device(at(piece), n, at(out), asynchronous=True))
        pos += n
    enc.sync()
    if caller:
        caller.sync()
        enc.set_stream(None)
        caller.close()
    return np.concatenate([o.reshape(-1)[: S * c * enc.frame_size].reshape(S, c, enc.frame_size) for (o, _), c in zip(outs, counts)], axis=1)


def at3_host_pipeline(enc, src, depth):
    """tests/test_gpu_parity.py's test_host_buffer_pipeline with AT3_CALLS blocks per call: page-locked buffers, inputs overwritten
    (NaN, or -1 in 16 bits) as soon as wait_input allows, outputs read and overwritten with 0xEE as soon as wait_frames allows"""
    piece = max(AT3_CALLS)
    ins = [enc.host_alloc((S, piece, 1024, 2), src.dtype) for _ in range(depth)]
    outs = [enc.host_alloc((S, piece, enc.frame_size), np.uint8) for _ in range(depth)]
    poison = -1 if src.dtype == np.int16 else np.nan
    got, counts, pos = [], [], 0

    def take(k):
        c = counts[k]
        got.append(outs[k % depth].reshape(-1)[: S * c * enc.frame_size].reshape(S, c, enc.frame_size).copy())
        outs[k % depth][...] = 0xEE

    for k, n in enumerate(AT3_CALLS):
        q = k % depth
        if k >= depth:
            enc.wait_input(depth - 1)
        ins[q][...] = poison
        flat = ins[q].reshape(-1)[: S * n * 2048].reshape(S, n, 1024, 2)   # the call's [S][n] layout at the buffer's start
        flat[...] = src[:, pos:pos + n]
        counts.append(enc.encode_host_async(flat, outs[q]))
        if k >= 1:
            enc.wait_input(1)   # the call before this one has left its buffer: poisoned at once
            ins[(k - 1) % depth][...] = poison
        if k >= depth - 1:
            enc.wait_frames(depth - 1)
            take(k - (depth - 1))
        pos += n
    enc.sync()
    for k in range(max(0, len(AT3_CALLS) - (depth - 1)), len(AT3_CALLS)):
        take(k)
    for a in ins + outs:
        enc.host_free(a)
    return np.concatenate(got, axis=1)


def at3enc(config):
    br, ng = {"lp2_gain": (b.LP2, 0), "lp2_nogain": (b.LP2, 1), "lp4_gain": (b.LP4, 0)}[config]
    nb = sum(AT3_CALLS)
    pcm, p16 = at3_signals(nb)
    exp = at3_expect(pcm, br, ng)
    decoy = np.ascontiguousarray(pcm[::-1])
    enc = b.At3Hip(n_streams=S, max_blocks=max(AT3_CALLS), bitrate=br, no_gain=ng, lib_path=EMU)
    runs = [("queued device calls", lambda: at3_queued(enc, pcm)),
            ("host pipeline depth 2", lambda: at3_host_pipeline(enc, pcm, 2)),
            ("host pipeline depth 4", lambda: at3_host_pipeline(enc, pcm, 4)),
            ("caller stream over a decoy", lambda: at3_queued(enc, pcm, decoy))]
    if config == "lp2_gain":
        runs += [("host pipeline depth 2 s16", lambda: at3_host_pipeline(enc, p16, 2)),
                 ("queued device calls, timing events", lambda: at3_queued(enc, pcm, timing=True))]
    for what, run in runs:
        t0 = time.time()
        enc.reset()
        got = run()
        report(f"at3enc {config} {what} ({got.shape[1]} of {exp.shape[1]} frames)", frames_bad(got, exp), t0)
    enc.close()


# ---- the ATRAC3plus encoder: its stream and the write stream ------------------------------------------------------------------
def at3penc(nch):
    from at3_testlib import at3p_signal, at3p_specs, at3p_write_frames
    calls = (2, 1, 3, 1)
    nf = sum(calls)
    t0 = time.time()
    names = ("mix", "burst")
    pcm = np.stack([np.stack([at3p_signal(n, nf, channel=c) for c in range(nch)], axis=-1) for n in names])
    exp = np.stack([at3p_write_frames(at3p_specs(n, nf, nch)) for n in names])
    enc = b.At3pHip(n_streams=2, max_frames=max(calls), channels=nch, lib_path=EMU)
    outs, pos = [], 0
    for n in calls:
        piece = np.ascontiguousarray(pcm[:, pos:pos + n])
        out = np.full((2, n, 2048), 0xEE, np.uint8)
        enc.encode_frames_device(at(piece), n, at(out), asynchronous=True)
        outs.append((out, piece))
        pos += n
    enc.sync()
    report(f"at3penc ch{nch} queued calls {calls}", frames_bad(np.concatenate([o for o, _ in outs], axis=1), exp), t0)
    enc.close()


def at3penc_tonal():
    """encode_frames_tonal, gated and shared, across three queued calls (the block carried from call to call), and
    write_frames_tonal behind a queued call"""
    import at3p_gha_lib as G
    import at3p_tonal_write_lib as L
    from at3_testlib import at3p_signal, at3p_specs, at3p_write_frames
    t0 = time.time()
    calls, nch = (2, 1, 2), 2
    nf = sum(calls)
    names = ("tones", "burst")
    pcm = np.stack([G.signal_pcm(n, nf, nch) for n in names])
    one = b.At3pHip(n_streams=1, max_frames=nf, channels=nch, lib_path=EMU)
    exp = np.stack([G.pipeline(pcm[s], True, True, write=lambda specs, recs: one.write_frames(specs[None], None, recs[None])[0])[0] for s in range(2)])
    one.close()
    enc = b.At3pHip(n_streams=2, max_frames=max(calls), channels=nch, lib_path=EMU)
    outs, pos = [], 0
    for n in calls:
        piece = np.ascontiguousarray(pcm[:, pos:pos + n])
        out = np.full((2, n, 2048), 0xEE, np.uint8)
        enc.encode_frames_tonal_device(at(piece), n, at(out), asynchronous=True, gated=True, shared=True)
        outs.append((out, piece))
        pos += n
    enc.sync()
    report(f"at3penc tonal gated shared queued calls {calls}", frames_bad(np.concatenate([o for o, _ in outs], axis=1), exp), t0)
    enc.close()
    t0 = time.time()
    g = np.load(L.GOLDEN)
    cid = L.writer_case_ids()[0]
    nch = int(cid.rsplit("_", 1)[1])
    blocks = L.blocks_from_ints(nch, g[f"{cid}_blocks"])
    flags = g[f"{cid}_flags"] if f"{cid}_flags" in g else None
    enc = b.At3pHip(n_streams=L.STREAMS, max_frames=L.FRAMES, channels=nch, lib_path=EMU)
    front = np.stack([np.stack([at3p_signal("mix", L.FRAMES, channel=c) for c in range(nch)], axis=-1)] * L.STREAMS)
    fout = np.full((L.STREAMS, L.FRAMES, 2048), 0xEE, np.uint8)
    enc.encode_frames_device(at(front), L.FRAMES, at(fout), asynchronous=True)
    got = enc.write_frames(L.case_specs(cid, int(g[f"{cid}_seed"])), flags, b.pack_tonal_blocks(blocks, nch))
    enc.sync()
    report(f"at3penc write_frames_tonal {cid} behind a queued call", frames_bad(got, g[f"{cid}_frames"]), t0)
    report("at3penc the queued call in front of it", frames_bad(fout, np.stack([at3p_write_frames(at3p_specs("mix", L.FRAMES, nch))] * L.STREAMS)))
    enc.close()


# ---- the ATRAC1 encoder -------------------------------------------------------------------------------------------------------
def at1enc():
    from at3_testlib import SIGNALS, at1_blocks, at1_oracle_encode
    t0 = time.time()
    calls = (4, 1, 1, 3, 1)
    nb = sum(calls)
    pcm = np.stack([at1_blocks(SIGNALS["mix"](nb // 2 + 1, seed=3), 2)[:nb], at1_blocks(SIGNALS["burst"](nb // 2 + 1), 2)[:nb]])
    exp = np.stack([at1_oracle_encode(pcm[i], "auto") for i in range(2)])
    enc = b.At1Hip(n_streams=2, max_blocks=max(calls), channels=2, lib_path=EMU)
    outs, pos = [], 0
    for n in calls:
        piece = np.ascontiguousarray(pcm[:, pos:pos + n])
        out = np.full((2, n, 2, 212), 0xEE, np.uint8)
        enc.encode_device(at(piece), n, at(out), asynchronous=True)
        outs.append((out, piece))
        pos += n
    enc.sync()
    got = np.concatenate([o for o, _ in outs], axis=1)
    report(f"at1enc queued calls {calls}", int((got != exp).any(axis=(2, 3)).sum()), t0)
    enc.close()


# ---- the single-stream engines: one scenario, an adapter per engine -----------------------------------------------------------
class Engine:
    """pieces: the inputs of two consecutive calls [S][n]...; call(in_ptr, k, out_ptr, flags) queues call k; room(k): an output
    array for call k; trim(out, k): its valid part; expect: the restatement's outputs of the two calls; extra(): further
    comparisons after the calls (the state the calls left), as [(what, bad)]"""
    eng = pieces = expect = None

    def set_stream(self, handle): self.eng._call("set_stream", ctypes.c_void_p(handle))
    def extra(self): return []
    def begin(self): pass


def scenario(name, e):
    def compare(what, outs, t0):
        bad = sum(frames_bad(e.trim(o, k), e.expect[k]) for k, o in enumerate(outs))
        report(f"{name} {what}", bad, t0)
        for w, bad in e.extra():
            report(f"{name} {what}: {w}", bad)

    # 1. the caller's stream: a queued producer over poison in front of each call, a queued copy of the result behind it
    t0 = time.time()
    e.eng.reset(); e.begin()
    caller = Caller()
    e.set_stream(caller.handle)
    outs, keep = [], []
    for k, piece in enumerate(e.pieces):
        src = np.ascontiguousarray(e.pieces[1 - k] if e.pieces[1 - k].shape == piece.shape else piece[::-1]).copy()   # valid, and not the input
        out, res = e.room(k), e.room(k)
        caller.copy(src, np.ascontiguousarray(piece))
        e.call(at(src), k, at(out), DEV | ASYNC)
        caller.copy(res, out)
        outs.append(res); keep += [src, out]
    caller.sync()
    e.set_stream(None)
    compare("caller stream, producer over poison", outs, t0)
    caller.close()
    # 2. two asynchronous host-memory calls back to back: one staging slot, results in pageable memory
    t0 = time.time()
    e.eng.reset(); e.begin()
    outs = [e.room(k) for k in range(2)]
    ins = [np.ascontiguousarray(p).copy() for p in e.pieces]
    for k in range(2):
        e.call(at(ins[k]), k, at(outs[k]), ASYNC)
        ins[k][...] = ins[k][::-1].copy() if ins[k].dtype == np.uint8 else 0   # pageable: read when the call was made
    e.eng.sync()
    compare("two queued host-memory calls", outs, t0)
    # 3. two asynchronous device-pointer calls
    t0 = time.time()
    e.eng.reset(); e.begin()
    outs = [e.room(k) for k in range(2)]
    ins = [np.ascontiguousarray(p).copy() for p in e.pieces]
    for k in range(2):
        e.call(at(ins[k]), k, at(outs[k]), DEV | ASYNC)
    e.eng.sync()
    compare("two queued device calls", outs, t0)
    e.eng.close()


class Decoder(Engine):
    def __init__(self, eng, frames, exp, cut, flags=0):
        self.eng, self.flags, self.cut = eng, flags, cut
        self.pieces = [np.ascontiguousarray(frames[:, :cut]), np.ascontiguousarray(frames[:, cut:])]
        self.expect = [np.ascontiguousarray(exp[:, :cut]), np.ascontiguousarray(exp[:, cut:])]

    def call(self, in_ptr, k, out_ptr, flags): self.eng.decode_ptr(in_ptr, self.pieces[k].shape[1], out_ptr, flags | self.flags)
    def room(self, k): return np.full(self.expect[k].shape, np.nan, np.float32)
    def trim(self, out, k): return out


def dec_at1():
    import at1_decode_lib as A1
    units = A1.fuzz_units(2, 2, 5, seed=42)
    exp, _ = A1.cpu_ref(A1.cpu_lib(), units)
    scenario("dec_at1", Decoder(b.At1HipDecoder(n_streams=2, max_frames=3, channels=2, lib_path=EMU), units, exp, 3))


def dec_at3():
    import at3_decode_lib as A3
    g = np.load(A3.GOLDEN)
    frames = A3.fuzz_frames(g, 192, 2, 5, seed=192)
    exp, _ = A3.cpu_ref(frames, 192, True)
    scenario("dec_at3", Decoder(b.At3HipDecoder(n_streams=2, frame_size=192, max_frames=3, lib_path=EMU), frames, exp, 2))


def dec_at3p():
    import at3p_tonal_lib as AT
    frames = AT.fuzz_tonal_streams(2, 2, 5, None)
    exp = np.stack([AT.cpu_tonal_decode(frames[i], 2)[0] for i in range(2)])
    scenario("dec_at3p tones", Decoder(b.At3pHipDecoder(n_streams=2, channels=2, max_frames=3, lib_path=EMU), frames, exp, 3, b.AT3PHIP_DECODE_TONES))


class Resampler(Engine):
    """two calls and the flush (extra(): host memory, blocking - it waits for what is queued)"""

    def __init__(self):
        import resample_lib as RS
        pair, C, T, cut = (48000, 44100), 2, 700, 450
        self.eng = b.HipResampler(*pair, channels=C, n_streams=2, max_in=cut, lib_path=EMU)
        xs = np.stack([RS.signal(k, T, C, seed=i, rate=pair[0]) for i, k in enumerate(("noise", "sweep"))])
        self.pieces = [np.ascontiguousarray(xs[:, :cut]), np.ascontiguousarray(xs[:, cut:])]
        refs = [RS.CpuResampler(*pair, C) for _ in range(2)]
        self.expect = [np.stack([refs[i].process(p[i]) for i in range(2)]) for p in self.pieces]
        self.tail = np.stack([refs[i].flush() for i in range(2)])
        self.n = [None, None]

    def call(self, in_ptr, k, out_ptr, flags): self.n[k] = self.eng.process_ptr(in_ptr, self.pieces[k].shape[1], out_ptr, flags)
    def room(self, k): return np.full((2, self.eng.max_out, 2), np.nan, np.float32)
    def trim(self, out, k): return self.eng._trim(out, self.expect[k].shape[1])
    def extra(self): return [("n_out", self.n != [x.shape[1] for x in self.expect]), ("flush", frames_bad(self.eng.flush(), self.tail))]


class Meter(Engine):
    """process twice, then finish (extra()); the calls have no output: room() is a token array"""

    def __init__(self):
        import loudness_lib as L
        self.L, C, T, cut = L, 2, L.HOP + 900, L.HOP - 300
        self.eng = b.HipLoudness(channels=C, n_streams=2, max_in=cut, max_hops=2, true_peak=True, lib_path=EMU)
        self.xs = np.stack([L.signal(k, T, C, seed=20 + i) for i, k in enumerate(("noise", "tone_dc"))])
        self.pieces = [np.ascontiguousarray(self.xs[:, :cut]), np.ascontiguousarray(self.xs[:, cut:])]
        self.expect = [np.zeros((2, 1, 1), np.float32)] * 2
        self.want_z = [L.hops(self.xs[i]) for i in range(2)]
        self.want = [L.measure(self.xs[i], True) for i in range(2)]

    def call(self, in_ptr, k, out_ptr, flags): self.eng.process_ptr(in_ptr, self.pieces[k].shape[1], flags & ~b.AT3HIP_OUT_ON_DEVICE)
    def room(self, k): return np.zeros((2, 1, 1), np.float32)
    def trim(self, out, k): return out

    def extra(self):
        z, res = self.eng.hops(), self.eng.finish()
        return [("hop sums", sum(not self.L.bits_equal(z[i], self.want_z[i]) for i in range(2))),
                ("results", sum(not self.L.results_equal(res[i], self.want[i]) for i in range(2)))]


class Apply(Engine):
    def __init__(self):
        import loudness_lib as L
        self.eng = b.HipLoudness(channels=2, n_streams=2, max_in=333, max_hops=1, lib_path=EMU)
        xs = np.stack([L.signal(k, 500, 2, seed=30 + i) for i, k in enumerate(("noise", "sweep"))])
        self.g = np.array([0.37, 2.5], np.float32)
        self.pieces = [np.ascontiguousarray(xs[:, :333]), np.ascontiguousarray(xs[:, 333:])]
        self.expect = [p * self.g[:, None, None] for p in self.pieces]

    def call(self, in_ptr, k, out_ptr, flags): self.eng.apply_ptr(in_ptr, self.pieces[k].shape[1], self.g, out_ptr, flags)
    def room(self, k): return np.full(self.pieces[k].shape, np.nan, np.float32)
    def trim(self, out, k): return out


class Limiter(Engine):
    """limit_start (begin()), limit twice, then limit_flush and the statistics (extra())"""

    def __init__(self):
        import limiter_lib as LM
        self.LM = LM
        T, cut = LM.TILE + 700, LM.TILE + 100
        xs, gains = LM.seven(T, 2)
        self.xs, self.gains = np.ascontiguousarray(xs[:2]), gains[:2]
        self.eng = b.HipLoudness(channels=2, n_streams=2, max_in=cut, max_hops=1, lib_path=EMU)
        res = [LM.restate(self.xs[i], self.gains[i], LM.CEIL, True) for i in range(2)]
        y, d = np.stack([r[0] for r in res]), LM.delay(True)
        self.stats = [r[3] for r in res]
        self.pieces = [np.ascontiguousarray(self.xs[:, :cut]), np.ascontiguousarray(self.xs[:, cut:])]
        self.expect = [np.ascontiguousarray(y[:, :cut - d]), np.ascontiguousarray(y[:, cut - d:T - d])]
        self.tail = np.ascontiguousarray(y[:, T - d:])
        self.n = [None, None]

    def begin(self): self.eng.limit_start(self.gains, self.LM.CEIL, True)
    def call(self, in_ptr, k, out_ptr, flags): self.n[k] = self.eng.limit_ptr(in_ptr, self.pieces[k].shape[1], out_ptr, flags)
    def room(self, k): return np.full(self.pieces[k].shape, np.nan, np.float32)
    def trim(self, out, k): return out.reshape(-1)[: self.expect[k].size].reshape(self.expect[k].shape)

    def extra(self):
        tail = self.eng.limit_flush()
        st = [(s.min_sum, s.n_limited) for s in self.eng.limit_stats()]
        return [("n_out", self.n != [x.shape[1] for x in self.expect]), ("flush", frames_bad(tail, self.tail)), ("statistics", st != self.stats)]


CASES = {"at3enc:lp2_gain": at3enc, "at3enc:lp2_nogain": at3enc, "at3enc:lp4_gain": at3enc, "at3penc:1": at3penc, "at3penc:2": at3penc,
         "at3penc_tonal": at3penc_tonal, "at1enc": at1enc, "dec_at1": dec_at1, "dec_at3": dec_at3, "dec_at3p": dec_at3p,
         "resampler": lambda: scenario("resampler", Resampler()), "meter": lambda: scenario("meter", Meter()),
         "apply": lambda: scenario("apply", Apply()), "limiter": lambda: scenario("limiter", Limiter())}

if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    unknown = [n for n in names if n not in CASES]
    if unknown or not names:
        sys.exit(f"usage: run_emu_streams.py [--nobuild] CASE ...; cases: {' '.join(CASES)}")
    if "--nobuild" not in sys.argv:
        run_emu.build(strict=True)
    os.environ.setdefault("EMU_STRICT", "1")
    print(f"streams mode: {mode()}", flush=True)
    for n in names:
        t = time.time()
        arg = n.split(":")[1:]
        CASES[n](*(int(a) if a.isdigit() else a for a in arg))
        print(f"{n} done ({time.time() - t:.1f}s)", flush=True)
