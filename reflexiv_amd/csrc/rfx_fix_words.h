// rfx_fix_words.h -- the word forms of the two contig fixing stages (rfx_fixing.hip, rfx_fixing2.hip): a contig read out of a
// packed record (rfx_dyn_packed) 32 bases at a time, and the owner search over scanned offsets.
// (fx_keep, fx_seg32, fx_cat32 and fx_find are the twins of rfx_dynamic.hip's dyn_keep, dyn_seg32, dyn_cat32 and dyn_find, which stay
// private to that file: the two copies must stay identical.)
#ifndef RFX_FIX_WORDS_H
#define RFX_FIX_WORDS_H
#include "rfx_internal.h"

namespace rfx {

#define FX_KW RFX_DYN_KEY_WORDS

// the first m of 32 bases, the rest 0
__device__ __forceinline__ uint64_t fx_keep(uint64_t x, int m) { return m >= 32 ? x : m <= 0 ? 0ull : x & ~(~0ull >> (2 * m)); }
// the 32 bases that start at base t of one packed segment of len bases (t < 0: the segment begins -t bases into the window); 0
// where the segment has no base -- the zero padding of the layout does the masking
__device__ __forceinline__ uint64_t fx_seg32(const uint64_t *__restrict__ w, int len, int t) {
    if (len <= 0 || t >= len || t <= -32) return 0ull;
    if (t < 0) return w[0] >> (2 * -t);
    const int wi = t >> 5, sh = (t & 31) * 2;
    uint64_t r = w[wi] << sh;
    if (sh && wi + 1 < ((len + 31) >> 5)) r |= w[wi + 1] >> (64 - sh);
    return r;
}
// a contig as its record holds it: key || extension for marker 1, extension || key otherwise
struct FxCat { const uint64_t *w0, *w1; int l0, l1; };
__device__ __forceinline__ FxCat fx_contig(const DynView &v, int64_t i) {
    const uint64_t *k = v.key + FX_KW * i, *e = v.ext + v.ext_off[i];
    const int kl = (int)v.key_len[i], el = v.ext_len[i];
    return v.marker[i] == 1 ? FxCat{k, e, kl, el} : FxCat{e, k, el, kl};
}
// the 32 bases that start at base t of the contig (0 past its end)
__device__ __forceinline__ uint64_t fx_cat32(const FxCat &c, int t) { return fx_seg32(c.w0, c.l0, t) | fx_seg32(c.w1, c.l1, t - c.l0); }
// the largest i < n with off[i] <= x (off[0] = 0 <= x): the record that owns word / item x; records of size 0 are skipped
__device__ __forceinline__ int64_t fx_find(const uint64_t *__restrict__ off, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace rfx
#endif
