"""k_psy's split flatness sum (flat_sums, atracdenc_amd/csrc/at3_k_backend.hpp) in the CPU SIMT harness, on BFUs constructed to sit on
both sides of its order-independence condition.

The reference adds a BFU's energies up as one f64 chain in line order (atrac_psy_common.cpp:167-178). The kernel adds them up in
chunks of sixteen lines, a lane per chunk, where every addition in every order is exact for the BFU's actual values - E_max - E_min
<= 29 - log2(lines) for the f32 exponent fields of its largest and smallest non-zero energies - and walks the chain
as one lane where not. Whichever way it goes the sum has to be the chain's, bit for bit; the test also restates the condition and
requires the kernel to have taken the path the condition names, and both paths to occur for both BFU sizes.

at3hip_debug_flat_sums exists in harness builds only.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from simt_harness_lib import build_strict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++ to compile the kernel sources for the host")


@pytest.fixture(scope="module")
def harness():
    return build_strict()


def energies(x):
    """e = (double)fmaxf(0, x * x) with the product an f32, as the kernel and the reference form them"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = (x * x).astype(np.float32)
    return np.where(e > 0, e, np.float32(0.0)).astype(np.float32)   # (fmaxf drops a NaN)


def chain_sum(e):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.cumsum(e.astype(np.float64), axis=1)[:, -1]        # (cumsum adds in order)


def order_free(e):
    """the condition, restated: True where any order of adding the row's energies is exact"""
    n = e.shape[1]
    field = (e.view(np.uint32) >> 23).astype(np.int64)
    ok = np.zeros(e.shape[0], bool)
    for i in range(e.shape[0]):
        nz = e[i] > 0
        if not nz.any():
            ok[i] = True
            continue
        f = np.maximum(field[i][nz], 1)
        ok[i] = f.max() < 255 and f.max() - f.min() <= 29 - int(np.log2(n))
    return ok


def with_exponent_span(rng, n, lines, span):
    """rows whose energies' exponent fields span exactly `span`: mantissas at random, the extremes pinned"""
    top = rng.randint(span + 2, 250, size=n)
    field = top[:, None] - rng.randint(0, span + 1, size=(n, lines))
    field[:, 0] = top
    field[np.arange(n), rng.randint(1, lines, size=n)] = top - span
    mant = rng.randint(0, 1 << 23, size=(n, lines)).astype(np.uint32)
    e = ((field.astype(np.uint32) << 23) | mant).view(np.float32)
    x = np.sqrt(e.astype(np.float64)).astype(np.float32)             # x * x lands within an ulp of e: the span is measured afterwards
    x *= rng.choice(np.float32([-1.0, 1.0]), size=x.shape)           # mixed signs of the lines
    return x


def cases(lines):
    rng = np.random.RandomState(1234 + lines)
    bound = 29 - int(np.log2(lines))
    rows = []
    rows.append(rng.randn(400, lines).astype(np.float32) * np.float32(0.05))                                 # noise-like: splits
    for span in (0, 1, bound - 2, bound - 1, bound, bound + 1, bound + 2, bound + 3, 40, 90):                # around the bound and far off
        rows.append(with_exponent_span(rng, 150, lines, span))
    z = rng.randn(120, lines).astype(np.float32)
    z[rng.rand(*z.shape) < 0.5] = 0.0                                                                         # zeros among the lines
    z[:10] = 0.0                                                                                              # all zero
    rows.append(z)
    d = (rng.randn(120, lines) * 1e-20).astype(np.float32)                                                    # energies in the f32 denormal range
    d[:40] *= np.float32(1e-3)                                                                                # ... and flushed to zero by the product
    d[40:80, 0] = np.float32(1e-17)                                                                           # one normal energy among denormals
    rows.append(d)
    h = rng.randn(160, lines).astype(np.float32) * np.float32(1e-3)
    h[:40, 0] = np.float32(3e18)                                                                              # one huge addend, first
    h[40:80, lines - 1] = np.float32(3e18)                                                                    # ... last
    h[80:120, 17] = np.float32(3e19)                                                                          # an energy that overflows to infinity
    h[120:140, 5] = np.float32(np.nan)                                                                        # a NaN line (its energy counts as zero)
    h[140:, 3] = np.float32(np.inf)
    rows.append(h)
    # chains that DO round differently when split: a large first addend, then many that are each half an ulp of the running sum
    r = np.full((60, lines), np.float32(2.0 ** -14), np.float32)
    r[:, 0] = np.float32(2.0 ** 13) * (np.float32(1.0) + rng.randint(0, 1 << 20, size=60).astype(np.float32) * np.float32(2.0 ** -23))
    r[:, 1:] *= (np.float32(1.0) + rng.randint(0, 1 << 22, size=(60, lines - 1)).astype(np.float32) * np.float32(2.0 ** -23))
    rows.append(r)
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)


@pytest.mark.parametrize("lines", [64, 32])
def test_split_sum_equals_the_chain_on_both_sides_of_the_condition(harness, lines):
    sys.path.insert(0, ROOT)
    from atracdenc_amd import binding as B
    lib = ctypes.CDLL(harness)
    fn = lib.at3hip_debug_flat_sums
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    x = cases(lines)
    n = x.shape[0]
    got = np.zeros(n, np.float64)
    chain = np.zeros(n, np.float64)
    split = np.full(n, -1, np.int32)
    enc = B.At3Hip(n_streams=1, max_blocks=2, lib_path=harness)
    assert fn(enc.ctx, x.ctypes.data, lines, n, got.ctypes.data, chain.ctypes.data, split.ctypes.data) == 0
    enc.close()
    e = energies(x)
    want = chain_sum(e)
    u64 = lambda a: np.ascontiguousarray(a).view(np.uint64)
    same = lambda a, b: (u64(a) == u64(b)) | (np.isnan(a) & np.isnan(b))
    assert same(chain, want).all(), np.argwhere(~same(chain, want))[:5].tolist()          # the kernel-side restatement of the chain is the chain
    bad = np.argwhere(~same(got, want))
    assert bad.size == 0, (bad[:5].tolist(), got[bad[0, 0]], want[bad[0, 0]], split[bad[0, 0]])
    free = order_free(e)
    assert np.array_equal(split == 1, free), np.argwhere((split == 1) != free)[:5].tolist()
    assert (split == 1).sum() > n // 4 and (split == 0).sum() > n // 4                     # both paths were taken, neither as an exception
    # the serial path is not decoration: among the rows that took it, adding chunk sums would have given other bits
    chunks = np.stack([chain_sum(e[:, 16 * c:16 * c + 16]) for c in range(lines // 16)], axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        by_chunks = np.cumsum(chunks, axis=1)[:, -1]
    differs = ~same(by_chunks, want)
    assert differs[split == 0].any() and not differs[split == 1].any()
