// rfx_packed_words.h -- the word helpers of every stage that works on packed record sets (rfx_dyn_packed: rfx_dynamic.hip,
// rfx_ksort.hip, rfx_reduce.hip, rfx_fixing.hip, rfx_fixing2.hip, rfx_endext.hip, rfx_ctgext.hip, rfx_endmap.hip) and of the contig de-duplication (rfx_dedup.hip),
// one definition each.  A packed sequence is 2 bits per base, 32 bases per 64-bit word, the first base in the two highest
// bits, every bit past the last base 0; a key is RFX_DYN_KEY_WORDS such words.  Everything in the first part is plain integer
// arithmetic, `__host__ __device__` and force-inlined on the device, so a host program can compile it with the two words defined
// away (tests/packed_words_main.cpp compares every helper with a byte model).  The last part, which needs the wave, is device-only.
#pragma once
#include <stdint.h>
#include "../../include/reflexiv_hip.h"

#ifdef __HIPCC__
#define PK_INLINE __forceinline__
#else
#define PK_INLINE inline
#endif

#define PK_KW RFX_DYN_KEY_WORDS      /* key words per record */
#define PK_CLAMP 30000               /* what buildingAlongFromThreeInt keeps of a left / right marker */

// ---- one word ---------------------------------------------------------------------------------------------------------------------
// the first m of 32 bases, the rest 0
__host__ __device__ PK_INLINE uint64_t pk_keep(uint64_t x, int m) { return m >= 32 ? x : m <= 0 ? 0ull : x & ~(~0ull >> (2 * m)); }
// the 32 two-bit groups of a word in reverse order: two swaps inside the bytes, then the bytes (one v_perm_b32 a half; the compiler
// does not find the byte swap in three more shift-and-mask steps)
__host__ __device__ PK_INLINE uint64_t pk_rev2(uint64_t x) {
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}
// a base code as its letter ("ACGT"), a letter as its code (A0 C1 G2, anything else 3), base t of a packed sequence
__host__ __device__ PK_INLINE uint32_t pk_letter(uint32_t code) { return (0x54474341u >> (8 * code)) & 0xFFu; }
__host__ __device__ PK_INLINE uint64_t pk_code(char ch) { return (uint64_t)(ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3); }
__host__ __device__ PK_INLINE uint32_t pk_base_of(const uint64_t *__restrict__ w, int t) { return (uint32_t)(w[t >> 5] >> (62 - 2 * (t & 31))) & 3u; }
__host__ __device__ PK_INLINE int32_t pk_clamp(int32_t v) { return v >= PK_CLAMP ? PK_CLAMP : v <= -PK_CLAMP ? -PK_CLAMP : v; }

// the letters of the 16 bases that start at base t of a packed sequence, as the 16 bytes of a text in four registers (the caller
// knows that the sequence has them: a word behind the last base is never read)
struct Pk16 { uint32_t a, b, c, d; };
__host__ __device__ PK_INLINE Pk16 pk_letters16(const uint64_t *__restrict__ w, int t) {
    const int wi = t >> 5, sh = (t & 31) * 2;
    uint64_t x = w[wi] << sh;
    if (sh > 32) x |= w[wi + 1] >> (64 - sh);
    const uint32_t y = (uint32_t)(x >> 32);
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) o[j >> 2] |= pk_letter((y >> (30 - 2 * j)) & 3u) << (8 * (j & 3));
    return Pk16{o[0], o[1], o[2], o[3]};
}

// ---- segments ---------------------------------------------------------------------------------------------------------------------
// the 32 bases that start at base t of one packed segment of len bases (t < 0: the segment begins -t bases into the window); 0
// where the segment has no base -- the zero padding of the layout does the masking.  One or two word loads and two shifts.
// (Positions are int: a record is bounded by 2^31 bases.  rfx_dedup_words.h keeps 64-bit forms for whole contigs.)
__host__ __device__ PK_INLINE uint64_t pk_seg32(const uint64_t *__restrict__ w, int len, int t) {
    if (len <= 0 || t >= len || t <= -32) return 0ull;
    if (t < 0) return w[0] >> (2 * -t);
    const int wi = t >> 5, sh = (t & 31) * 2;
    uint64_t r = w[wi] << sh;
    if (sh && wi + 1 < ((len + 31) >> 5)) r |= w[wi + 1] >> (64 - sh);
    return r;
}
// among the first m of the 32 bases of a and b, the positions at which the two differ (compared on codes: either bit of a pair)
__host__ __device__ PK_INLINE int pk_mismatch32(uint64_t a, uint64_t b, int m) {
    const uint64_t x = pk_keep(a ^ b, m);
    return __builtin_popcountll((x | (x >> 1)) & 0x5555555555555555ull);
}
// the 32 bases that start at base t (0 <= t < len) of the REVERSE COMPLEMENT of a segment of len bases, 0 behind its last base: base
// x of it is 3 - base len - 1 - x of the segment, so the window is the segment's 32 bases from len - t - 32, turned round and
// complemented.  Nothing at or past base len of the segment is used, so the segment needs no zero padding (a read of the read store)
__host__ __device__ PK_INLINE uint64_t pk_rc_seg32(const uint64_t *__restrict__ w, int len, int t) {
    return pk_keep(pk_rev2(~pk_seg32(w, len, len - t - 32)), len - t);
}
// a contig as its record holds it: key || extension for marker 1, extension || key otherwise (V: DynView, or a host stand-in)
struct FxCat { const uint64_t *w0, *w1; int l0, l1; };
template <class V>
__host__ __device__ PK_INLINE FxCat fx_contig(const V &v, int64_t i) {
    const uint64_t *k = v.key + PK_KW * i, *e = v.ext + v.ext_off[i];
    const int kl = (int)v.key_len[i], el = v.ext_len[i];
    return v.marker[i] == 1 ? FxCat{k, e, kl, el} : FxCat{e, k, el, kl};
}
// the 32 bases that start at base t of the contig (0 past its end)
__host__ __device__ PK_INLINE uint64_t fx_cat32(const FxCat &c, int t) { return pk_seg32(c.w0, c.l0, t) | pk_seg32(c.w1, c.l1, t - c.l0); }

// the largest i < n with off[i] <= x (off[0] = 0 <= x): the record that owns word / byte / item x of a scan; entries of size 0 are
// skipped
template <class T>
__host__ __device__ PK_INLINE int64_t pk_find(const T *__restrict__ off, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- a key in four named registers, never an indexed array --------------------------------------------------------------------------
struct Pk4 { uint64_t w0, w1, w2, w3; };
__host__ __device__ PK_INLINE uint64_t pk_word(const Pk4 &a, int j) { return j == 0 ? a.w0 : j == 1 ? a.w1 : j == 2 ? a.w2 : j == 3 ? a.w3 : 0ull; }
__host__ __device__ PK_INLINE void pk_or(Pk4 &a, int j, uint64_t v) {
    a.w0 |= j == 0 ? v : 0ull; a.w1 |= j == 1 ? v : 0ull; a.w2 |= j == 2 ? v : 0ull; a.w3 |= j == 3 ? v : 0ull;
}
// base p (0..127) of four words / a base code at position p of a word set
__host__ __device__ PK_INLINE uint64_t pk_base(const Pk4 &a, int p) { return (pk_word(a, p >> 5) >> (62 - 2 * (p & 31))) & 3ull; }
__host__ __device__ PK_INLINE uint64_t pk_at(uint64_t code, int p) { return code << (62 - 2 * (p & 31)); }
// the 128 bases moved s bases (0..127) towards the front, zeros behind
__host__ __device__ PK_INLINE Pk4 pk_shl(const Pk4 &a, int s) {
    const int ws = s >> 5, bs = (s & 31) * 2;
    Pk4 r;
    uint64_t lo;
    lo = pk_word(a, ws + 1); r.w0 = (pk_word(a, ws) << bs) | (bs ? lo >> (64 - bs) : 0ull);
    lo = pk_word(a, ws + 2); r.w1 = (pk_word(a, ws + 1) << bs) | (bs ? lo >> (64 - bs) : 0ull);
    lo = pk_word(a, ws + 3); r.w2 = (pk_word(a, ws + 2) << bs) | (bs ? lo >> (64 - bs) : 0ull);
    r.w3 = pk_word(a, ws + 3) << bs;
    return r;
}
// the first len bases kept, everything behind them 0
__host__ __device__ PK_INLINE Pk4 pk_keep4(const Pk4 &a, int len) {
    return Pk4{pk_keep(a.w0, len), pk_keep(a.w1, len - 32), pk_keep(a.w2, len - 64), pk_keep(a.w3, len - 96)};
}
// the first len (0..128) bases in reverse order at the front, zeros behind: reverse all 128 groups (the bases are then the LAST
// len), move them to the front
__host__ __device__ PK_INLINE Pk4 pk_reverse(const Pk4 &a, int len) {
    const Pk4 rv{pk_rev2(a.w3), pk_rev2(a.w2), pk_rev2(a.w1), pk_rev2(a.w0)};
    return len <= 0 ? Pk4{0, 0, 0, 0} : pk_keep4(pk_shl(rv, 128 - len), len);
}
// dynamicSubKmerComparator: the shorter key is a prefix of the longer one (the padding is 0 on both sides)
__host__ __device__ PK_INLINE bool pk_prefix(const Pk4 &x, int lx, const Pk4 &y, int ly) {
    const int m = lx < ly ? lx : ly;
    const Pk4 a = pk_keep4(x, m), b = pk_keep4(y, m);
    return a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2 && a.w3 == b.w3;
}
__host__ __device__ PK_INLINE Pk4 pk_load(const uint64_t *__restrict__ key, int64_t i) {
    const uint64_t *p = key + PK_KW * i;
    return Pk4{p[0], p[1], p[2], p[3]};
}
__host__ __device__ PK_INLINE void pk_store(uint64_t *__restrict__ key, int64_t i, const Pk4 &a) {
    uint64_t *p = key + PK_KW * i;
    p[0] = a.w0; p[1] = a.w1; p[2] = a.w2; p[3] = a.w3;
}

// the reverse complement of the first len (0..128) bases at the front, zeros behind: the complemented padding turns up ahead of the
// bases and is shifted out
__host__ __device__ PK_INLINE Pk4 pk_revcomp(const Pk4 &a, int len) { return pk_reverse(Pk4{~a.w0, ~a.w1, ~a.w2, ~a.w3}, len); }
// a k-mer as the counter writes it (rfx_dev_count_reads_ragged / _ragged_w: k / 32 full words of 32 bases, then one word with the
// k % 32 last bases in its LOWEST bits; k <= 31 is that word alone) as a key: k = 1..127, zeros behind the last base; whatever the
// last word holds above its bases is dropped, and a word the format does not have (k % 32 == 0: none behind the full ones) is not read
__host__ __device__ PK_INLINE Pk4 pk_from_counter(const uint64_t *__restrict__ w, int k) {
    const int f = k >> 5, res = k & 31;
    const uint64_t last = res ? w[f] << (64 - 2 * res) : 0ull;
    return Pk4{f > 0 ? w[0] : last, f > 1 ? w[1] : f == 1 ? last : 0ull, f > 2 ? w[2] : f == 2 ? last : 0ull, f == 3 ? last : 0ull};
}
// what DynamicKmerBinarizer reads out of the decimal text of a count c >= 0: ten digits or more are 1,000,000,000
__host__ __device__ PK_INLINE int64_t pk_count_as_text(int64_t c) { return c >= 1000000000LL ? 1000000000LL : c; }

// ---- the decimal text of an int, and an int out of text ---------------------------------------------------------------------------
// (32-bit unsigned arithmetic: 0u - (uint32_t)v is |v| for every int, INT_MIN included)
__host__ __device__ PK_INLINE int pk_int_chars(int v) {               // characters of std::to_string(v)
    uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    int c = v < 0 ? 2 : 1;
    while (a >= 10) { a /= 10; c++; }
    return c;
}
__host__ __device__ PK_INLINE char pk_int_char(int v, int q) {        // its character q
    if (v < 0) { if (q == 0) return '-'; q--; }
    uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    int c = 1;
    for (uint32_t t = a; t >= 10; t /= 10) c++;
    for (int s = c - 1 - q; s > 0; s--) a /= 10;
    return (char)('0' + a % 10);
}
// one number of an attribute "m|l|r" in t[i, e): an optional sign, digits (the value stops growing at nine of them), one '|' behind
// it stepped over; no digits read as 0.  i is left behind what was read
__host__ __device__ PK_INLINE int pk_parse_int(const char *__restrict__ t, int64_t &i, int64_t e) {
    bool neg = false;
    if (i < e && (t[i] == '-' || t[i] == '+')) { neg = t[i] == '-'; i++; }
    long long v = 0;
    while (i < e && t[i] >= '0' && t[i] <= '9') { if (v < 100000000LL) v = v * 10 + (t[i] - '0'); i++; }
    if (i < e && t[i] == '|') i++;
    return (int)(neg ? -v : v);
}

// what pk_parse_int reads out of the text pk_int_char writes for v: v itself up to nine digits, the first nine of ten
__host__ __device__ PK_INLINE int pk_int_as_text(int v) {
    const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v, t = a >= 1000000000u ? a / 10u : a;
    return v < 0 ? -(int)t : (int)t;
}

// a decimal int in t[p, e), p left behind its digits.  sign: '-' allowed; plus: '+' too (Integer.parseInt); canon: as
// Integer.toString writes it (no leading zero, no "-0").  false: no int there
__host__ __device__ PK_INLINE bool pk_dec_int(const char *__restrict__ t, int64_t &p, int64_t e, bool sign, bool plus, bool canon, int *out) {
    bool neg = false;
    if (p < e && ((sign && t[p] == '-') || (plus && t[p] == '+'))) { neg = t[p] == '-'; p++; }
    const int64_t d0 = p;
    int64_t v = 0;
    while (p < e && t[p] >= '0' && t[p] <= '9' && p - d0 < 11) { v = v * 10 + (t[p] - '0'); p++; }
    const int nd = (int)(p - d0);
    if (nd == 0 || nd > 10) return false;
    if (canon && ((nd > 1 && t[d0] == '0') || (neg && v == 0))) return false;
    if (neg) v = -v;
    if (v < -2147483648LL || v > 2147483647LL) return false;
    *out = (int)v;
    return true;
}

// ---- device only ------------------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
// the shortest and the longest key of a launch into *min_len / *max_len (CallFlags, rfx_internal.h); every thread of the wave calls it
__device__ __forceinline__ void pk_note_lengths(uint32_t *min_len, uint32_t *max_len, bool live, int len) {
    uint32_t lo = live ? (uint32_t)len : 0xFFFFFFFFu, hi = live ? (uint32_t)len : 0u;
    for (int d = 32; d > 0; d >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
    }
    // one wave, one pair of atomics -- and only while they would still move the value: min and max are monotone, so a plain
    // (possibly stale) read can only ask for an atomic too many.  With every wave of 9 million records hitting the two words, the
    // unconditional form cost 3.3 ms a launch
    if ((threadIdx.x & 63) == 0) {
        if (lo < *(const volatile uint32_t *)min_len) atomicMin(min_len, lo);
        if (hi > *(const volatile uint32_t *)max_len) atomicMax(max_len, hi);
    }
}
#endif
