// Bitstream primitives shared by the device code of the three codecs (gfx950): the sequential MSB-first reader of the ATRAC3 and
// ATRAC3plus decoders, the linear prefix-code scan, the sign extension and the split atomicOr core of the three bit writers.
// Each is a rule of a bitstream the project reproduces bit for bit, so each is written once. Device-only, all inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace at3 {

// The low n bits of v as a two's-complement number (MakeSign); n in 1..32.
__device__ __forceinline__ int sext(uint32_t v, int n) { return (int)(v << (32 - n)) >> (32 - n); }

// MSB-first sequential reader over a unit or frame staged in LDS as big-endian words; a read must end within `limit` bits, and
// one that would not sets `bad` and yields 0, as does every read after it. The two words around the read position are kept in a
// register (`win` = words wi, wi + 1): a read costs no LDS access but the one refill when it crosses into the next word.
// Preconditions, for every function:
//   - n is in 1..32 for peek and rd (peek(0) would shift by 64) and in 0..32 for advance, which so crosses at most one word;
//   - `words` has two readable zero words behind the data: peek looks up to 32 bits past the limit, and the refill on
//     entering word wi loads word wi + 1.
struct MsbReader {
    const uint32_t* w;
    int pos, limit, bad, wi;
    uint64_t win;
    __device__ __forceinline__ MsbReader(const uint32_t* words, int limit_bits)
        : w(words), pos(0), limit(limit_bits), bad(0), wi(0), win(((uint64_t)words[0] << 32) | words[1]) {}
    __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)((win << (pos - 32 * wi)) >> (64 - n)); }
    __device__ __forceinline__ void advance(int n)
    {
        pos += n;
        if ((pos >> 5) != wi) {
            ++wi;
            win = (win << 32) | w[wi + 1];
        }
    }
    __device__ __forceinline__ uint32_t rd(int n)
    {
        if (bad || pos + n > limit) {
            bad = 1;
            return 0;
        }
        const uint32_t v = peek(n);
        advance(n);
        return v;
    }
};

// One symbol of a prefix code of NSYM symbols and at most 8 bits, found by a linear scan of tab[sym] = len << 12 | code (len 0: no
// code). No match sets `invalid`; a match that ends past the limit sets b.bad. Both return 0.
template <int NSYM>
__device__ __forceinline__ int prefix_scan(MsbReader& b, const uint16_t* tab, int& invalid)
{
    if (b.bad) return 0;
    const uint32_t v = b.peek(8);
    for (int sym = 0; sym < NSYM; ++sym) {
        const int len = tab[sym] >> 12, code = tab[sym] & 0xfff;
        if (len && (int)(v >> (8 - len)) == code) {
            if (b.pos + len > b.limit) {
                b.bad = 1;
                return 0;
            }
            b.advance(len);
            return sym;
        }
    }
    invalid = 1;
    return 0;
}

// ORs the n bits of val (nothing set above them) into an MSB-first bit string held in big-endian words, at bit `pos`, split over
// two words where it has to be. No guard and no mask: n is in 1..32, word (pos + n - 1) >> 5 exists, and the caller's words start
// out zero. Lanes may write neighbouring fields of one word at once, hence the atomics.
__device__ __forceinline__ void or_bits_msb(uint32_t* words, int pos, uint32_t val, int n)
{
    const int w = pos >> 5, off = pos & 31;
    const int room = 32 - off;
    if (n <= room) {
        atomicOr(&words[w], val << (room - n));
    } else {
        atomicOr(&words[w], val >> (n - room));
        atomicOr(&words[w + 1], val << (32 - (n - room)));
    }
}

}  // namespace at3
