#!/usr/bin/env python3
"""DEVELOPMENT HARNESS: the HOST code of every engine (the three encoders and decoders, the resampler, the meter with its
limiter, the ATRAC3plus tone analysis, the ATRAC3 stage-level entry points) through the CPU SIMT emulator (tools/emu) with its call trace on
(EMU_TRACE, hip/hip_runtime.h): which runtime call, on which stream, with which event, byte count and launch geometry. Each
case runs one fixed script of calls in a child process and its trace is compared with tests/golden/host_trace/<case>.txt -
the driver of tests/test_host_call_trace.py. `--write` writes the goldens instead. The samples are silence: the host code
never looks at them. Runs of event creations with consecutive ordinals are folded into one line. Up to `# destroy` the order
of the calls is compared; of *_destroy, every wait and every release it makes (each sorted: the order among them says nothing).
The joint-stereo-with-gain and the one-channel case differ from the first one in their launches only and run a short script."""
import ctypes, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
import numpy as np
import run_emu

GOLDEN = os.path.join(ROOT, "tests", "golden", "host_trace")
DEV = 1 | 2   # AT3HIP_PCM_ON_DEVICE | AT3HIP_OUT_ON_DEVICE: in the harness any host array is "device" memory
CALLER = 0x1000   # a stream handle the harness did not make (never dereferenced)
S = 2


def destroy(enc):
    with open(os.environ["EMU_TRACE"], "a") as f:   # (the harness appends and flushes line by line)
        f.write("# destroy\n")
    enc.close()


def at3_case(bitrate, no_gain, channels=2, prime_only=False, short=False):
    def run():
        from atracdenc_amd import binding as b
        enc = b.At3Hip(n_streams=S, max_blocks=4, bitrate=bitrate, no_gain=no_gain, channels=channels, lib_path=run_emu.EMU)
        f32 = np.zeros((S, 4, 1024, channels), np.float32)
        i16 = np.zeros((S, 4, 1024, channels), np.int16)
        out = np.zeros((S, 4, enc.frame_size), np.uint8)
        if prime_only:   # one block on a fresh context: nothing but the look-ahead is primed (n_out == 0)
            enc.encode(f32[:, :1])
            destroy(enc)
            return
        enc.encode(f32[:, :3]); enc.encode(f32[:, :2])                 # host float: the priming call, then parity 1
        if short:   # one host int16 call, one queued call on device pointers
            enc.encode_s16(i16[:, :2])
            enc.encode_device(f32.ctypes.data, 2, out.ctypes.data, asynchronous=True); enc.sync()
            enc.reset()
            destroy(enc)
            return
        enc.encode_s16(i16[:, :2]); enc.encode_s16(i16[:, :2])         # host int16, both parities
        for _ in range(3): enc.encode_device(f32.ctypes.data, 2, out.ctypes.data, asynchronous=True)
        enc.wait_input(1); enc.wait_frames(1); enc.sync()
        enc.set_stream(CALLER); enc.encode_device(f32.ctypes.data, 2, out.ctypes.data); enc.set_stream(0)
        enc.set_option(b.OPT_GAIN_FORM, b.GAIN_FORM_ONE_WAVE); enc.encode_device(f32.ctypes.data, 2, out.ctypes.data)
        enc.set_option(b.OPT_GAIN_FORM, b.GAIN_FORM_TWO_WAVES)
        enc.set_option(b.OPT_TIMING_EVERY, 2)
        for _ in range(3): enc.encode_device(f32.ctypes.data, 2, out.ctypes.data)
        enc.reset()
        destroy(enc)
    return run


def at1_case():
    from atracdenc_amd import binding as b
    enc = b.At1Hip(n_streams=S, max_blocks=2, channels=2, lib_path=run_emu.EMU)
    f32 = np.zeros((S, 2, 512, 2), np.float32)
    out = np.zeros((S, 2, 2, 212), np.uint8)
    enc.encode(f32); enc.encode(f32[:, :1])
    enc.encode_s16(np.zeros((S, 2, 512, 2), np.int16))
    enc.encode_device(f32.ctypes.data, 2, out.ctypes.data, asynchronous=True); enc.sync()
    enc.read_tap(b.At1Hip.TAP_MASKS, np.int32, (S, 2, 2))
    enc.reset()
    destroy(enc)


def at3p_case():
    from atracdenc_amd import binding as b
    enc = b.At3pHip(n_streams=S, max_frames=2, channels=2, lib_path=run_emu.EMU)
    at = lambda a: a.ctypes.data
    pcm = np.zeros((S, 2, 2048, 2), np.float32)
    bands = enc.pqf(pcm)
    specs = enc.mdct(bands)
    enc.pqf_mdct(pcm)
    frames = enc.write_frames(specs)
    enc.pqf_ptr(at(pcm), 2, at(bands), DEV)
    enc.mdct_ptr(at(bands), 2, None, at(specs), DEV)
    enc.pqf_mdct_ptr(at(pcm), 2, None, at(bands), at(specs), DEV)
    enc.write_frames_ptr(at(specs), 2, None, at(frames), DEV)
    for _ in range(3): enc.encode_frames_device(pcm.ctypes.data, 2, frames.ctypes.data, asynchronous=True)
    enc.sync()
    enc.encode_frames_s16(np.zeros((S, 2, 2048, 2), np.int16))
    enc.reset()
    destroy(enc)


def decoder_case(kind):
    def run():
        from atracdenc_amd import binding as b
        dec = {"at1": lambda: b.At1HipDecoder(n_streams=S, max_frames=2, channels=2, lib_path=run_emu.EMU),
               "at3": lambda: b.At3HipDecoder(n_streams=S, frame_size=384, max_frames=2, lib_path=run_emu.EMU),
               "at3p": lambda: b.At3pHipDecoder(n_streams=S, max_frames=2, channels=2, lib_path=run_emu.EMU)}[kind]()
        src, dst = dec._shapes()
        frames = np.zeros((S, 2) + src, np.uint8)
        out = np.zeros((S, 2) + dst, np.float32)
        at = lambda a: a.ctypes.data
        dec.decode(frames); dec.decode(frames[:, :1], s16=True)                       # host float, host int16
        dec.decode_ptr(at(frames), 2, at(out), DEV | b.AT3HIP_ASYNC); dec.sync()      # device pointers, queued
        dec.decode_ptr(at(frames), 2, at(out), DEV)
        if kind == "at3p": dec.decode(frames, tones=True)
        dec.counters(reset=True)
        dec._call("set_stream", ctypes.c_void_p(CALLER)); dec.decode_ptr(at(frames), 1, at(out), DEV); dec._call("set_stream", None)
        dec.reset()
        destroy(dec)
    return run


def resampler_case():
    from atracdenc_amd import binding as b
    r = b.HipResampler(48000, 44100, channels=2, n_streams=S, max_in=64, lib_path=run_emu.EMU)
    f32 = np.zeros((S, 64, 2), np.float32)
    i16 = np.zeros((S, 64, 2), np.int16)
    out = np.zeros((S, r.max_out, 2), np.float32)
    at = lambda a: a.ctypes.data
    r.process_ptr(at(f32), 64, at(out), DEV)                          # device in and out: no staging yet
    r.flush()                                                         # to host: the output staging is the flush's
    r.process(f32); r.process(f32[:, :32], out_s16=True)              # host float in, float and int16 out
    r.process_s16(i16)                                                # host int16 in
    r.process_ptr(None, 0, at(out), 0)                                # an empty call
    r.flush_ptr(at(out), b.AT3HIP_OUT_ON_DEVICE)
    r.reset()
    destroy(r)


def meter_case(true_peak):
    def run():
        from atracdenc_amd import binding as b
        m = b.HipLoudness(channels=2, n_streams=S, max_in=4500, max_hops=4, true_peak=true_peak, lib_path=run_emu.EMU)
        f32 = np.zeros((S, 4500, 2), np.float32)
        i16 = np.zeros((S, 4500, 2), np.int16)
        out = np.zeros((S, 64, 2), np.float32)
        gains = np.ones(S, np.float32)
        at = lambda a: a.ctypes.data
        m.process(f32)                                                # host float: one hop
        if true_peak:   # the short script: the converter's launches and the table of create
            m.process_ptr(at(f32), 64, b.AT3HIP_PCM_ON_DEVICE | b.AT3HIP_ASYNC); m.sync()
            m.finish()
            m.reset()
            destroy(m)
            return
        m.process_s16(i16[:, :100])                                   # host int16
        m.process_ptr(at(f32), 4410, b.AT3HIP_PCM_ON_DEVICE)          # device
        m.process_ptr(None, 0, 0)                                     # an empty call
        m.hops(); m.finish()
        m.apply(f32[:, :64], gains); m.apply_s16(i16[:, :64], gains)  # host float, host int16
        m.apply_ptr(at(f32), 64, gains, at(out), DEV); m.apply_ptr(at(out), 64, gains, at(out), DEV)   # device, and in place
        m.reset()
        destroy(m)
    return run


def limiter_case():
    from atracdenc_amd import binding as b
    m = b.HipLoudness(channels=2, n_streams=S, max_in=512, max_hops=4, true_peak=False, lib_path=run_emu.EMU)
    f32 = np.zeros((S, 512, 2), np.float32)
    i16 = np.zeros((S, 512, 2), np.int16)
    out = np.zeros((S, 512, 2), np.float32)
    gains = np.ones(S, np.float32)
    at = lambda a: a.ctypes.data
    m.limit_start(gains, 0.5, true_peak=True)                         # the first start: the buffers and the converter's table
    m.limit(f32); m.limit_s16(i16[:, :300])                           # host float, host int16
    m.limit_ptr(at(f32), 512, at(out), DEV)
    m.limit_flush(); m.limit_stats()
    m.limit_start(gains, 0.5)                                         # a second start allocates nothing
    m.limit(f32)
    m.limit_flush_ptr(at(out), b.AT3HIP_OUT_ON_DEVICE); m.limit_stats()
    destroy(m)


def at3p_tones_case():
    from atracdenc_amd import binding as b
    enc = b.At3pHip(n_streams=S, max_frames=2, channels=2, lib_path=run_emu.EMU)
    at = lambda a: a.ctypes.data
    pcm = np.zeros((S, 2, 2048, 2), np.float32)
    bands = np.zeros((S, 2, 2, 16, 128), np.float32)
    resid = np.zeros_like(bands)
    frames = np.zeros((S, 2, 2048), np.uint8)
    for gated, shared in ((False, False), (True, False), (False, True)):
        enc.analyse_tones(bands, gated=gated, shared=shared)
        enc.analyse_tones_device(at(bands), 2, at(resid), gated=gated, shared=shared)
    enc.encode_frames_tonal(pcm); enc.encode_frames_tonal_s16(np.zeros((S, 2, 2048, 2), np.int16))
    for _ in range(2): enc.encode_frames_tonal_device(at(pcm), 2, at(frames), asynchronous=True)
    enc.sync()
    one = {"nb": 1, "shared": [False], "leader": False,
           "bands": [[{"start": None, "stop": None, "waves": [(100, 20, 0)]}], [{"start": None, "stop": None, "waves": []}]]}
    enc.write_frames(np.zeros((S, 2, 2, 2048), np.float32), tonal=b.pack_tonal_blocks([[one, None]] * S, 2))
    enc.reset()
    destroy(enc)


def at3_stage_case():
    from atracdenc_amd import binding as b
    enc = b.At3Hip(n_streams=S, max_blocks=2, bitrate=b.LP2, lib_path=run_emu.EMU)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    curves = lambda n, per: (np.zeros(n * per, np.int32), np.zeros((n * per, 8), np.int32), np.zeros((n * per, 8), np.int32))
    enc.mdct(np.zeros((1, 4, 512), np.float32)); enc.mdct(np.zeros((1, 4, 512), np.float32), *curves(1, 4))
    enc.mdct(np.zeros((1, 4, 512), np.float32), max_levels=True)
    ges = lambda n, *cv: enc.gain_energy_scale(np.zeros((n, 256), np.float32), np.zeros((n, 256), np.float32), np.zeros(n, np.float32), *cv)
    ges(2); ges(2, *curves(2, 1))
    ges(16)                                                           # more than any call before: the staging grows
    enc.mdct(np.zeros((6, 4, 512), np.float32), *curves(6, 4), max_levels=True)   # and again
    bands, specs, mx = np.zeros((2, 4, 512), np.float32), np.zeros((2, 1024), np.float32), np.zeros((2, 4), np.float32)
    cv = curves(2, 4)
    enc._call("mdct", vp(bands), vp(specs), None, None, None, 2, DEV)               # device pointers
    enc._call("mdct_levels", vp(bands), vp(specs), vp(mx), *[vp(a) for a in cv], 2, DEV)
    po, ps, out = np.zeros((2, 256), np.float32), np.zeros(2, np.float32), np.zeros((2, 4), np.float32)
    cv = curves(2, 1)
    enc._call("gain_energy_scale", vp(po), vp(po), None, None, None, vp(ps), vp(out), 2, DEV)
    enc._call("gain_energy_scale", vp(po), vp(po), *[vp(a) for a in cv], vp(ps), vp(out), 2, DEV)
    enc.set_option(b.OPT_QUANT_TAP, 1); enc.set_option(b.OPT_QUANT_TAP, 0); enc.set_option(b.OPT_QUANT_TAP, 1)   # the one early release
    destroy(enc)


def cases():
    from atracdenc_amd.binding import LP2, LP4
    return {"at3_lp2_gain": at3_case(LP2, 0), "at3_lp2_nogain": at3_case(LP2, 1), "at3_lp4_gain": at3_case(LP4, 0, short=True),
            "at3_lp4_nogain": at3_case(LP4, 1), "at3_mono_lp2": at3_case(LP2, 0, channels=1, short=True),
            "at3_prime_gain": at3_case(LP2, 0, prime_only=True), "at3_prime_nogain": at3_case(LP2, 1, prime_only=True),
            "at1": at1_case, "at3p": at3p_case,
            "dec_at1": decoder_case("at1"), "dec_at3": decoder_case("at3"), "dec_at3p": decoder_case("at3p"),
            "resampler": resampler_case, "meter": meter_case(False), "meter_true_peak": meter_case(True), "limiter": limiter_case,
            "at3p_tones": at3p_tones_case, "at3_stage": at3_stage_case}


def fold(lines):
    """event_create / event_destroy lines with consecutive ordinals and equal flags become `event_create e4..e259 flags=0`"""
    out, run = [], None   # run: [verb, first, last, rest]
    def flush():
        if run: out.append(f"{run[0]} e{run[1]}{'..e%d' % run[2] if run[2] != run[1] else ''}{run[3]}")
    for ln in lines:
        m = re.fullmatch(r"(event_create|event_destroy) e(\d+)(.*)", ln)
        if m and run and run[0] == m.group(1) and run[3] == m.group(3) and int(m.group(2)) == run[2] + 1:
            run[2] += 1
            continue
        flush()
        run = [m.group(1), int(m.group(2)), int(m.group(2)), m.group(3)] if m else None
        if not m: out.append(ln)
    flush()
    return out


def canonical(lines):
    cut = lines.index("# destroy")
    key = lambda ln: (ln.split()[0], [int(n) for n in re.findall(r"\d+", ln)])
    waits = sorted((ln for ln in lines[cut + 1:] if "sync" in ln), key=key)
    releases = sorted((ln for ln in lines[cut + 1:] if "sync" not in ln), key=key)
    return fold(lines[:cut + 1]) + waits + fold(releases)


def trace_of(case):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "trace.txt")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", case], env=dict(os.environ, EMU_TRACE=path), cwd=ROOT)
        with open(path) as f:
            return canonical(f.read().splitlines())


if __name__ == "__main__":
    if "--child" in sys.argv:
        cases()[sys.argv[sys.argv.index("--child") + 1]]()
        sys.exit(0)
    if "--nobuild" not in sys.argv: run_emu.build()
    write = "--write" in sys.argv
    for case in [a for a in sys.argv[1:] if not a.startswith("--")] or list(cases()):
        got = trace_of(case)
        golden = os.path.join(GOLDEN, case + ".txt")
        if write:
            os.makedirs(GOLDEN, exist_ok=True)
            with open(golden, "w") as f:
                f.write("\n".join(got) + "\n")
            print(f"{case}: wrote {len(got)} lines")
            continue
        with open(golden) as f:
            want = f.read().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        bad = sum(a != b for a, b in zip(got, want)) + abs(len(got) - len(want))
        head = next(i for i, ln in enumerate(got) if not ln.startswith("stream_create"))
        print(f"{case}: begins with {'; '.join(got[:head])}; then {got[head].split()[0]}")
        print(f"{case}: {len(got)} calls traced, golden {len(want)}: bad {bad}")
        if bad:
            for i in range(max(0, first - 3), min(max(len(got), len(want)), first + 6)):
                print(f"  line {i + 1}: got  {got[i] if i < len(got) else '-'}\n  {' ' * len(str(i + 1))}       want {want[i] if i < len(want) else '-'}")
