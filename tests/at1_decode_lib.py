"""Helpers of the ATRAC1 decoder's tests, golden generator and benchmark (TEST INFRASTRUCTURE: nothing under atracdenc_amd/
imports this module).

  * CpuDecoder: the C restatement tests/host/at1_decode_cpu.c, compiled on first use into a temporary directory with the
    reference's arithmetic flags (gcc -O2 -ffp-contract=off -fno-fast-math).
  * ref_decode: the REAL reference decoder (TAtrac1Decoder of oracle/_ref/libat3ref.so) run by a small driver that binds three
    of the library's exported symbols by their mangled names - no reference header is included, no reference source is copied.
  * crafted_units / write_aea / read_wav: inputs and files of the tests.
"""
import ctypes
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

from at3_testlib import REF_SO, _vp

HERE = os.path.dirname(os.path.abspath(__file__))
CPU_SRC = os.path.join(HERE, "host", "at1_decode_cpu.c")
CFLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
UNIT = 212
GOLDEN = os.path.join(HERE, "golden", "at1_decode.npz")


def build_cpu_decoder(outdir):
    so = os.path.join(str(outdir), "libat1decode_cpu.so")
    subprocess.check_call(["gcc", "-std=gnu11", *CFLAGS, "-shared", "-o", so, CPU_SRC, "-lm"])
    return so


_cpu_so = None


def cpu_lib(outdir=None):
    """ctypes handle of the restatement (built once per process, into `outdir` or a fresh temporary directory)."""
    global _cpu_so
    if _cpu_so is None:
        _cpu_so = build_cpu_decoder(outdir or tempfile.mkdtemp(prefix="at1dec_"))
    lib = ctypes.CDLL(_cpu_so)
    lib.at1d_state_bytes.restype = ctypes.c_size_t
    lib.at1d_reset.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.at1d_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


class CpuDecoder:
    """One stream of the C restatement; state carries across decode() calls like a TAtrac1Decoder's."""

    def __init__(self, channels, lib=None):
        self.lib = lib or cpu_lib()
        self.nch = channels
        self.state = np.zeros(self.lib.at1d_state_bytes() * channels, np.uint8)
        self.rejected = np.zeros(2, np.uint64)
        self.reset()

    def reset(self):
        self.lib.at1d_reset(_vp(self.state), self.nch)
        self.rejected[:] = 0

    def decode(self, units):
        """units [N][C][212] uint8 -> pcm [N][512][C] float32"""
        units = np.ascontiguousarray(units, np.uint8)
        assert units.ndim == 3 and units.shape[1:] == (self.nch, UNIT), units.shape
        pcm = np.zeros((units.shape[0], 512, self.nch), np.float32)
        self.lib.at1d_decode(_vp(self.state), self.nch, _vp(units), units.shape[0], _vp(pcm), _vp(self.rejected))
        return pcm


def cpu_decode(units):
    """[N][C][212] -> ([N][512][C] float32, rejected-frame count) from start-of-stream state"""
    d = CpuDecoder(units.shape[1])
    pcm = d.decode(units)
    return pcm, int(d.rejected.sum())


# ---- the real reference decoder ----------------------------------------------------------------------------------------------
# The driver declares the three entry points with layout-compatible stand-ins (a unique_ptr is one pointer; std::function's
# layout does not depend on its signature; EProcessResult is an int-sized enum) and gives them the reference's mangled
# names. It decodes n_frames blocks of 512 samples, calling the lambda once per block exactly as TPCMEngine does.
REF_DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
struct UPtr { void* p; ~UPtr() {} };
struct Meta { const uint16_t channels; };
extern UPtr create_aea_input(const std::string&) asm("_Z14CreateAeaInputRKNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEE");
extern void decoder_ctor(void* self, UPtr* in) asm("_ZN10NAtracDEnc14TAtrac1DecoderC1EOSt10unique_ptrI16ICompressedInputSt14default_deleteIS2_EE");
extern std::function<int(float*, const Meta&)> decoder_lambda(void* self) asm("_ZN10NAtracDEnc14TAtrac1Decoder9GetLambdaEv");
int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const int nch = atoi(argv[2]), n = atoi(argv[3]);
    UPtr in = create_aea_input(argv[1]);
    void* self = calloc(1, 1 << 20);   // more than sizeof(TAtrac1Decoder); the object is never destroyed
    decoder_ctor(self, &in);
    std::function<int(float*, const Meta&)> fn = decoder_lambda(self);
    std::vector<float> buf(512 * nch);
    const Meta meta = {(uint16_t)nch};
    FILE* out = fopen(argv[4], "wb");
    for (int f = 0; f < n; ++f) {
        fn(buf.data(), meta);
        fwrite(buf.data(), sizeof(float), buf.size(), out);
    }
    fclose(out);
    return 0;
}
"""

_ref_driver = None


def have_ref_decoder():
    return os.path.exists(REF_SO)


def ref_driver(outdir=None):
    global _ref_driver
    if _ref_driver is None:
        d = outdir or tempfile.mkdtemp(prefix="at1dref_")
        src = os.path.join(d, "at1_ref_decode.cpp")
        with open(src, "w") as f:
            f.write(REF_DRIVER)
        exe = os.path.join(d, "at1_ref_decode")
        libdir = os.path.dirname(REF_SO)
        subprocess.check_call(["g++", "-std=c++17", "-O2", src, "-o", exe, f"-L{libdir}", "-lat3ref", f"-Wl,-rpath,{libdir}"])
        _ref_driver = exe
    return _ref_driver


def write_ref_aea(path, units):
    """AEA file through the reference's own writer (at3ref_write_container kind 3). TAeaOutput writes a zero 'dummy' unit in
    place of the first one it is handed (aea.cpp:163-189): the unit sequence in the file is `units` with units[0, 0] zeroed,
    which this returns."""
    n, nch = units.shape[:2]
    lib = ctypes.CDLL(REF_SO)
    flat = np.ascontiguousarray(units.reshape(-1, UNIT))
    rc = lib.at3ref_write_container(3, path.encode(), _vp(flat), flat.shape[0], UNIT, 0, n, nch)
    assert rc == 0
    seq = units.copy()
    seq[0, 0] = 0
    return seq


def ref_decode(units, workdir=None):
    """The reference decoder over `units` [N][C][212] (first unit zeroed, see write_ref_aea): returns (unit sequence decoded,
    pcm [N][512][C] float32, rejected-frame reasons as printed on stderr)."""
    n, nch = units.shape[:2]
    d = workdir or tempfile.mkdtemp(prefix="at1dref_run_")
    aea, raw = os.path.join(d, "in.aea"), os.path.join(d, "out.f32")
    seq = write_ref_aea(aea, units)
    r = subprocess.run([ref_driver(), aea, str(nch), str(n), raw], capture_output=True, text=True, check=True)
    pcm = np.fromfile(raw, np.float32).reshape(n, 512, nch)
    reasons = [ln for ln in r.stderr.splitlines() if ln.startswith("Skipping invalid ATRAC1 frame: ")]
    if workdir is None:
        shutil.rmtree(d)
    return seq, pcm, reasons


# ---- crafted sound units -------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.buf = bytearray(UNIT)
        self.pos = 0

    def put(self, v, n):
        for k in range(n - 1, -1, -1):
            if self.pos < UNIT * 8 and (v >> k) & 1:
                self.buf[self.pos >> 3] |= 0x80 >> (self.pos & 7)
            self.pos += 1


def make_unit(bsm=(2, 2, 0), bfu_idx=7, wl=None, sf=None, mantissa=None):
    """A sound unit from its fields: bsm = the three raw 2-bit block-size fields (low, mid, high), wl / sf per BFU (52 entries,
    only the first BfuAmountTab[bfu_idx] are written), mantissa(bfu, i, wordlen) -> raw bits. Bits past 1696 are dropped."""
    nbfu = [20, 28, 32, 36, 40, 44, 48, 52][bfu_idx]
    wl = list(wl) if wl is not None else [0] * 52
    sf = list(sf) if sf is not None else [0] * 52
    w = BitWriter()
    for v in bsm:
        w.put(v, 2)
    w.put(0, 2)
    w.put(bfu_idx, 3)
    w.put(0, 5)
    for i in range(nbfu):
        w.put(wl[i], 4)
    for i in range(nbfu):
        w.put(sf[i], 6)
    spb = [8, 8, 8, 8, 4, 4, 4, 4, 8, 8, 8, 8, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 9, 9, 9, 9, 10, 10, 10, 10,
           12, 12, 12, 12, 12, 12, 12, 12, 20, 20, 20, 20, 20, 20, 20, 20]
    for b in range(nbfu):
        if wl[b]:
            n = wl[b] + 1
            for i in range(spb[b]):
                w.put(mantissa(b, i, n) & ((1 << n) - 1) if mantissa else 0, n)
    return np.frombuffer(bytes(w.buf), np.uint8)


def set_block_modes(units, modes):
    """Overwrite the block-size fields of units [N][C][212] with modes [N][C][3] (raw 2-bit field values)."""
    u = units.copy()
    m = np.asarray(modes, np.uint8)
    u[..., 0] = (m[..., 0] << 6) | (m[..., 1] << 4) | (m[..., 2] << 2) | (u[..., 0] & 3)
    return u


def crafted_units(nch, seed):
    """Malformed and extreme sound units, [N][nch][212]: every invalid block-size field, allocations that read past the 212
    bytes, units that fill the bit budget with maximum word lengths at the largest scale factor (decoded far beyond +-1), and
    seeded random bytes."""
    rng = np.random.default_rng(seed)
    units = []
    for lo, mi in ((3, 2), (2, 3), (3, 3), (3, 0), (1, 3)):
        for hi in range(4):
            units.append(make_unit((lo, mi, hi)))
    for idx in (0, 3, 7):   # every BFU at word length 16: the mantissas need far more than the unit's 1696 bits
        units.append(make_unit((2, 2, 0), idx, wl=[15] * 52, sf=[63] * 52, mantissa=lambda b, i, n: 0x5555))
    # just past the end: 20 BFUs, enough word-length-16 BFUs to end one bit beyond the unit
    units.append(make_unit((2, 2, 0), 0, wl=[15] * 8 + [0] * 44, sf=[63] * 52))
    for k, bsm in enumerate(((2, 2, 0), (0, 0, 3), (1, 1, 1), (2, 0, 2))):
        # the bit budget filled with maximum word lengths, scale factor 63 (2^0): clamps to +-1
        wl = [15 if b < 9 else 0 for b in range(52)]
        units.append(make_unit(bsm, 0, wl=wl, sf=[63] * 52, mantissa=lambda b, i, n, k=k: (0x7fff if (b + i + k) % 2 else 0x8001)))
        units.append(make_unit(bsm, 7, wl=[3] * 52, sf=[63 - (b % 5) for b in range(52)],
                               mantissa=lambda b, i, n: int(rng.integers(0, 1 << n))))
    units += [rng.integers(0, 256, UNIT, dtype=np.uint8) for _ in range(24)]
    units = np.stack(units)
    n = (len(units) + nch - 1) // nch * nch
    units = np.concatenate([units, rng.integers(0, 256, (n - len(units), UNIT), dtype=np.uint8)])
    return np.ascontiguousarray(units.reshape(-1, nch, UNIT))


def random_modes(shape, rng):
    """Valid block-size fields: low / mid in 0..2, high in 0..3 (LogCount 2, 1, 0 / 3, 2, 1, 0)."""
    return np.stack([rng.integers(0, 3, shape), rng.integers(0, 3, shape), rng.integers(0, 4, shape)], -1)


# ---- the fuzz inputs of the GPU tests and of the SIMT-harness tests (the same bytes from the same seeds) ----------------------
def fuzz_units(nch, n_streams, n_frames, seed):
    """valid reference-shaped units (the goldens' encoder output with rewritten block sizes) mixed with random and malformed ones"""
    rng = np.random.default_rng(seed)
    g = np.load(GOLDEN)
    pool = np.concatenate([g[f"{n}_units"] for n in g["cases"] if f"_ch{nch}" in n and not n.startswith("random")])
    pool = np.concatenate([pool, crafted_units(nch, seed)])
    idx = rng.integers(0, pool.shape[0], (n_streams, n_frames))
    units = pool[idx]
    units = np.where(rng.random((n_streams, n_frames, 1, 1)) < 0.5, set_block_modes(units, random_modes(units.shape[:3], rng)), units)
    noise = rng.integers(0, 256, units.shape, dtype=np.uint8)
    return np.where(rng.random((n_streams, n_frames, 1, 1)) < 0.25, noise, units).astype(np.uint8)


def cpu_ref(cpu, units):
    """[S][N][C][212] -> ([S][N][512][C], rejected counts summed over streams)"""
    outs, rej = [], np.zeros(2, np.uint64)
    for s in range(units.shape[0]):
        d = CpuDecoder(units.shape[2], cpu)
        outs.append(d.decode(units[s]))
        rej += d.rejected
    return np.stack(outs), rej.tolist()


# ---- files -----------------------------------------------------------------------------------------------------------------
def write_aea(path, units, title=b"test"):
    """An AEA file holding exactly `units` [N][C][212] (the layout TAeaInput reads: 2048-byte header, then the units)."""
    n, nch = units.shape[:2]
    hdr = bytearray(2048)
    hdr[1] = 0x08
    hdr[4:4 + len(title)] = title
    hdr[260:264] = struct.pack("<I", n)
    hdr[264] = nch
    with open(path, "wb") as f:
        f.write(bytes(hdr))
        f.write(np.ascontiguousarray(units, np.uint8).tobytes())


def read_wav(path):
    """(header fields, samples int16 [frames][channels]) of a canonical 44-byte PCM WAV"""
    data = open(path, "rb").read()
    riff, size, wave, fmt, fmt_len, tag, nch, rate, brate, align, bits, dtag, dlen = struct.unpack("<4sI4s4sIHHIIHH4sI", data[:44])
    h = dict(riff=riff, size=size, wave=wave, fmt=fmt, fmt_len=fmt_len, tag=tag, nch=nch, rate=rate, byte_rate=brate,
             align=align, bits=bits, data=dtag, data_len=dlen, file_len=len(data))
    return h, np.frombuffer(data[44:44 + dlen], "<i2").reshape(-1, nch)


def s16_of(pcm):
    """the float -> 16-bit rule of the decoder's s16 output and of at3hipenc -d: lrintf(x * 32767.0f)"""
    return np.rint(pcm.astype(np.float32) * np.float32(32767.0)).astype(np.int16)
