// rfx_dedup_words.h -- the word helpers of the contig de-duplication (rfx_dedup.hip).  A contig is 2 bits
// per base, 32 bases per 64-bit word, the first base in the two highest bits, every bit past the last base 0
// (rfx_contigs_packed).  Everything here is plain integer arithmetic on such words and is `__host__ __device__`, so a host
// program can compile it with the two words defined away (tests/dedup_words_main.cpp compares every helper with a byte model).
#pragma once
#include <stdint.h>
#include "rfx_packed_words.h"     // pk_rev2.  Positions here are 64-bit (a contig is not bounded by 2^31 bases), so dd_keep / dd_seg32 stay

// the first m of 32 bases, the rest 0
__host__ __device__ inline uint64_t dd_keep(uint64_t x, int64_t m) { return m >= 32 ? x : m <= 0 ? 0ull : x & ~(~0ull >> (2 * m)); }

// the 32 bases that start at base t of a contig of len bases (t < 0: the contig begins -t bases into the window); 0 where the
// contig has no base -- the zero padding of the layout does the masking.  One or two word loads and two shifts.
__host__ __device__ inline uint64_t dd_seg32(const uint64_t *w, int64_t len, int64_t t) {
    if (len <= 0 || t >= len || t <= -32) return 0ull;
    if (t < 0) return w[0] >> (2 * -t);
    const int64_t wi = t >> 5;
    const int sh = (int)(t & 31) * 2;
    uint64_t r = w[wi] << sh;
    if (sh && wi + 1 < ((len + 31) >> 5)) r |= w[wi + 1] >> (64 - sh);
    return r;
}
// the same window of the reverse complement: the forward window that ends at len - t, reversed by 2-bit groups and
// complemented, 0 past the end
__host__ __device__ inline uint64_t dd_seg32_rc(const uint64_t *w, int64_t len, int64_t t) {
    if (len <= 0 || t >= len || t < 0) return 0ull;
    return dd_keep(~pk_rev2(dd_seg32(w, len, len - 32 - t)), len - t);
}
__host__ __device__ inline uint64_t dd_strand32(const uint64_t *w, int64_t len, int rc, int64_t t) {
    return rc ? dd_seg32_rc(w, len, t) : dd_seg32(w, len, t);
}

// a piece of a contig: bases [from, from + n) of the strand `rc` of the contig (w, len)
struct DdSeg { const uint64_t *w; int64_t len, from, n; int32_t rc, pad; };
// the 32 bases that start at base u of the piece (u > -32: the piece begins -u bases into the window), 0 past its end
__host__ __device__ inline uint64_t dd_piece32(const DdSeg &s, int64_t u) {
    if (s.n <= 0 || u >= s.n || u <= -32) return 0ull;
    if (u >= 0) return dd_keep(dd_strand32(s.w, s.len, s.rc, s.from + u), s.n - u);
    return dd_keep(dd_strand32(s.w, s.len, s.rc, s.from), s.n) >> (2 * -u);
}
// the 32 bases that start at base t (>= 0) of the concatenation a + b: long + flank, flank + long, or a plain copy (b.n = 0)
__host__ __device__ inline uint64_t dd_cat32(const DdSeg &a, const DdSeg &b, int64_t t) { return dd_piece32(a, t) | dd_piece32(b, t - a.n); }

// the marker 31-mer at base p (p + 31 <= len): 31 bases above the 01 pair; and the 31-mer of its reverse complement
// (binaryLongReverseComplementary :2877-2906)
__host__ __device__ inline uint64_t dd_mer31(const uint64_t *w, int64_t len, int64_t p) { return (dd_seg32(w, len, p) & ~3ull) | 1ull; }
__host__ __device__ inline uint64_t dd_mer31_rc(uint64_t m) { return (~pk_rev2(m) << 2) | 1ull; }

// the 15-mer seed at base p (>= 0) of a strand of a contig of n bases.  Past the end the block's 01 terminator reads as one C,
// then A's (what (int)(leftShiftOutFromArray(leftShiftArray(c, p), 15)[0] >>> 2*(32-15)) yields there): with zero padding
// that is one added bit when p <= n < p + 15
__host__ __device__ inline uint32_t dd_seed15(const uint64_t *w, int64_t n, int64_t p, int rc) {
    uint32_t x = (uint32_t)(dd_strand32(w, n, rc, p) >> 34);
    if (p <= n && n < p + 15) x |= 1u << (28 - 2 * (int)(n - p));
    return x;
}
