// rfx_dynamic.hip -- the dynamic-k record format and passes on the GPU:
// P/ReflexivDSDynamicKmerFirstFour.java (DynamicKmerBinarizerFromReducedToSubKmer :2931-3016, DSkmerRandomReflection
// :2509-2762, DSExtendReflexivKmer :1581-2373, DSBinarySubKmerWithShortExtensionToString :226-263) and
// P/ReflexivDSDynamicKmerIteration.java (its binarizer, DSExtendReflexivKmerToArrayLoop :465-1249, ...LongExtensionToString).
//
// The third record layout -- keys of ANY length as left-aligned 31-base blocks with a 01 terminator, an attribute long
// (marker << 62 | left << 32 | right, negatives as 30000 - v), extensions in the same left-aligned form -- is what a Row
// carries.  In HBM a record set is PACKED (rfx_dyn_packed): four 64-bit key words per record and
// word-aligned extensions, 32 bases per word, first base in the two highest bits, every bit past the last base 0 and every
// unused key word 0.  Every producer here writes those zeros; every consumer compares whole words and relies on them.
// The 31-base blocks are formed (by shifts, from the words) only where the reference's behaviour depends on them: the ORDER
// of sort("k-1") (array<long>: element by element as signed longs, a proper prefix first).
//
// One pass = the scan of SURVEY.md B.5 with a one-row holder, except that a row meets the holder when their keys are EQUAL
// OR ONE IS A PREFIX OF THE OTHER (dynamicSubKmerComparator), so equal-key runs are no longer the unit of work.  What is:
// a FAMILY -- a maximal run of sorted rows that agree on their first Lmin bases, Lmin = the shortest key of the set.  A row
// can only be related to an earlier row through a common prefix of at least Lmin bases, and everything between two related
// rows shares that prefix, so no holder ever survives a family boundary.  Kernels: k_dyn_keys (the sort keys and the set's
// shortest / longest key), the library's stable radix sort (block count, then the blocks the set has, last to first),
// k_dyn_heads, k_dyn_walk<COUNT / WRITE> (the owner of a family head walks it with the reference's rules; the decisions do
// not depend on the toggling orientation, which is the parity of the emission rank inside the partition: a prefix sum, as on
// the fixed-k path), k_dyn_sizes (lengths, attributes and word counts of the emissions), and k_dyn_emit_key / k_dyn_emit_ext:
// ONE THREAD PER OUTPUT WORD, which reads its 32 bases from the concatenation of up to three packed segments (dyn_cat32).
// The gather behind the sort is the same emission with "copy" descriptors.  No pass needs more records or more extension
// words than its input (a flip keeps both lengths, a merge gives ceil((a+b)/32) <= ceil(a/32) + ceil(b/32)), so the output
// of a pass is allocated from its input's sizes and no host wait sits between the sizes and the emission.
#include <algorithm>
#include <string>
#include <vector>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

#define DYN_KW PK_KW                        /* key words per record */
#define DYN_MAXB 4                          // 31-base blocks per key: keys up to 124 bases (the reference's k-mer list ends at 95)
#define DYN_MAXK (31 * DYN_MAXB)

// (DynDev, DynView, DynOut, dyn_view and dyn_out: rfx_internal.h -- rfx_ksort.hip works on the same sets)
// (the functions defined as rfx::... are the ones rfx_ksort.hip shares: rfx_internal.h declares them)
int rfx::dyn_alloc(rfx_ctx *ctx, DynDev &d, int64_t n, int64_t words) {
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    RFX_ALLOC(d.key, uint64_t, m * DYN_KW);
    RFX_HIP(d.key_len.alloc(m, ctx->stream));
    RFX_ALLOC(d.ext, uint64_t, std::max<int64_t>(words, 1));
    RFX_ALLOC(d.ext_off, uint64_t, n + 1);
    RFX_ALLOC(d.ext_len, int32_t, m);
    RFX_ALLOC(d.marker, int32_t, m);
    RFX_ALLOC(d.left, int32_t, m);
    RFX_ALLOC(d.right, int32_t, m);
    d.n = n; d.words = words;
    return RFX_OK;
}
namespace {

// ---- words ----------------------------------------------------------------------------------------------------------------
// (pk_keep, pk_seg32, pk_find, the integer text and the flags of a call: rfx_packed_words.h, rfx_internal.h)
// up to three packed segments, each a word pointer and a length in bases: key + ext, ext + key, P + L + S of a merge
struct DynCat { const uint64_t *w0, *w1, *w2; int l0, l1, l2; };
// the 32 bases that start at base t of the concatenation (0 past its end)
__device__ __forceinline__ uint64_t dyn_cat32(const DynCat &c, int t) {
    return pk_seg32(c.w0, c.l0, t) | pk_seg32(c.w1, c.l1, t - c.l0) | pk_seg32(c.w2, c.l2, t - c.l0 - c.l1);
}
// the first n (<= 124) bases of two keys are equal: whole words, then one masked word
__device__ __forceinline__ bool dyn_prefix_equal(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, int n) {
    if (n > DYN_MAXK) n = DYN_MAXK;
    const int fw = n >> 5, r = n & 31;
    for (int j = 0; j < DYN_KW - 1; j++) if (j < fw && a[j] != b[j]) return false;
    return r == 0 || pk_keep(a[fw] ^ b[fw], r) == 0;
}
__device__ __forceinline__ bool dyn_keys_equal(const uint64_t *__restrict__ key, const uint8_t *__restrict__ len, int64_t a, int64_t b) {
    const uint64_t *x = key + DYN_KW * a, *y = key + DYN_KW * b;
    return len[a] == len[b] && x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3];
}
// what is wrong with a call's input (CallFlags::bad): a key longer than 124 bases, offsets that run backwards
enum { DYN_TOO_LONG = 1, DYN_BAD_OFFSETS = 2 };
// the set's shortest / longest key into the flags; a key past DYN_MAXK is refused
__device__ __forceinline__ void dyn_note_lengths(CallFlags *__restrict__ flags, bool live, int len) {
    pk_note_lengths(&flags->min_len, &flags->max_len, live, len);
    if (live && len > DYN_MAXK) atomicOr(&flags->bad, (uint32_t)DYN_TOO_LONG);
}

// block j of a key from its words: bases 31 j .. 31 j + 30 in bits 63..2, the 01 terminator behind the last base of the last
// block (bit 0 when that block is full) -- what Row carries and rfx_dyn_bases_to_blocks writes
__device__ __forceinline__ uint64_t dyn_block(const uint64_t *__restrict__ w, int len, int j) {
    const int b0 = 31 * j;
    int m = len - b0;
    if (m > 31) m = 31;
    uint64_t x = pk_seg32(w, len, b0) & ~3ull;
    if (b0 + 31 >= len) x |= 1ull << (2 * (31 - m));
    return x;
}
// sort keys: block j with the sign bit flipped (Spark compares signed longs), 0 past the last block; the block count; and the
// set's shortest and longest key.  blk == nullptr: the lengths only (the operators that do not sort)
__global__ __launch_bounds__(256) void k_dyn_keys(const uint64_t *__restrict__ key, const uint8_t *__restrict__ key_len, int64_t n,
                                                  uint64_t *__restrict__ blk /* [DYN_MAXB][n] */, uint64_t *__restrict__ nblk,
                                                  uint32_t *__restrict__ perm, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const int len = live ? (int)key_len[i] : 0;
    dyn_note_lengths(flags, live, len);
    if (!live || !blk) return;
    const int use = len > DYN_MAXK ? DYN_MAXK : len;
    const int nb = use <= 0 ? 1 : (use - 1) / 31 + 1;
    const uint64_t *w = key + DYN_KW * i;
    for (int j = 0; j < DYN_MAXB; j++) blk[(int64_t)j * n + i] = j < nb ? (dyn_block(w, use, j) ^ 0x8000000000000000ull) : 0ull;
    nblk[i] = (uint64_t)nb;
    perm[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_dyn_gather_u64(const uint64_t *__restrict__ src, const uint32_t *__restrict__ perm, int64_t n,
                                                        uint64_t *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// logical partition p starts at floor(p*n/P), moved forward past equal keys (the order contract)
__global__ void k_dyn_part_starts(const uint64_t *__restrict__ key, const uint8_t *__restrict__ key_len, int64_t n, int P, int64_t *__restrict__ ps) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t prev = 0;
    for (int p = 0; p < P; p++) {
        int64_t s = (int64_t)p * n / P;
        if (s < prev) s = prev;
        while (s > 0 && s < n && dyn_keys_equal(key, key_len, s, s - 1)) s++;
        ps[p] = s; prev = s;
    }
    ps[P] = n;
}

// a row heads a family when it opens a partition or differs from its predecessor inside the first lmin bases
__global__ __launch_bounds__(256) void k_dyn_heads(const uint64_t *__restrict__ key, int64_t n, const int64_t *__restrict__ ps, int P,
                                                   uint32_t lmin, uint32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool h = i == 0;
    for (int p = 0; p <= P && !h; p++) h = ps[p] == i;
    if (!h) h = !dyn_prefix_equal(key + DYN_KW * i, key + DYN_KW * (i - 1), (int)lmin);
    head[i] = h ? 1u : 0u;
}

// an emission: the source record(s) and what is done with them (the orientation is decided by the emission's rank)
struct DynDesc { int32_t kind; int32_t bubble; int64_t a, b; };    // kind 0: flip record a; 1: merge forward a + reflected b; 2: copy a

struct DynRow { const uint64_t *key; int klen; int elen; int marker, left, right; int64_t idx; };

__device__ __forceinline__ DynRow dyn_row(const DynView &v, int64_t q) {
    DynRow r;
    r.key = v.key + DYN_KW * q; r.klen = (int)v.key_len[q]; r.elen = v.ext_len[q];
    r.marker = v.marker[q]; r.left = v.left[q]; r.right = v.right[q]; r.idx = q;
    return r;
}
// equal, or one a prefix of the other
__device__ __forceinline__ bool dyn_related(const DynRow &a, const DynRow &b) {
    return dyn_prefix_equal(a.key, b.key, a.klen < b.klen ? a.klen : b.klen);
}

// DSExtendReflexivKmer.call (FirstFour:1603-1763) / DSExtendReflexivKmerToArrayLoop.call (Iteration:487-...) over one family.
// WRITE = false: counts the family's emissions into cnt[head]; WRITE = true: writes descriptors at base[head] + rank.
template <bool WRITE>
__global__ __launch_bounds__(128) void k_dyn_walk(const DynView v, int64_t n, const uint32_t *__restrict__ head, int stage, int start_iteration,
                                                  uint32_t *__restrict__ cnt, const uint64_t *__restrict__ base, DynDesc *__restrict__ desc) {
    const int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q0 >= n) return;
    if (!head[q0]) { if (!WRITE) cnt[q0] = 0; return; }
    uint32_t rank = 0;
    const uint64_t b0 = WRITE ? base[q0] : 0;
    auto emit = [&](int kind, int64_t a, int64_t b, int bubble) {
        if (WRITE) desc[b0 + rank] = DynDesc{kind, bubble, a, b};
        rank++;
    };
    bool have = false;
    DynRow h{};
    for (int64_t q = q0; q < n && (q == q0 || !head[q]); q++) {
        const DynRow s = dyn_row(v, q);
        if (!have) { h = s; have = true; continue; }
        if (!dyn_related(s, h)) { emit(0, h.idx, -1, 0); h = s; continue; }
        if (s.marker == h.marker) { emit(0, s.idx, -1, 0); continue; }
        if (s.marker == 1) {
            const int extra = h.klen < s.klen ? s.klen - h.klen : 0;
            if (s.klen < h.klen) {                               // the forward row is the shorter one: no merge
                if (stage == 0 || start_iteration < 61) emit(0, s.idx, -1, 0);
                continue;
            }
            int d; bool ok = true;
            if (s.left < 0 && h.right < 0) d = -1;
            else if (s.left >= 0 && h.right >= 0) d = -1;
            else if (s.left >= 0 && s.left - h.elen >= 0) d = s.left - h.elen;
            else if (h.right >= 0 && h.right - s.elen - extra >= 0) d = h.right - s.elen;
            else { ok = false; d = 0; }
            if (!ok) { emit(0, s.idx, -1, 0); continue; }
            emit(1, s.idx, h.idx, d); have = false;
        } else {
            const int extra = s.klen < h.klen ? h.klen - s.klen : 0;
            if (h.klen < s.klen) {                               // the forward HOLDER is the shorter one
                if (stage == 1 && start_iteration >= 61) have = false;
                emit(0, s.idx, -1, 0);
                continue;
            }
            int d; bool ok = true;
            if (s.right < 0 && h.left < 0) d = -1;
            else if (s.right >= 0 && h.left >= 0) d = -1;
            else if (s.right >= 0 && s.right - h.elen - extra >= 0) d = s.right - h.elen;
            else if (h.left >= 0 && h.left - s.elen >= 0) d = h.left - s.elen;
            else { ok = false; d = 0; }
            if (!ok) { emit(0, s.idx, -1, 0); continue; }
            emit(1, h.idx, s.idx, d); have = false;
        }
    }
    if (have) emit(0, h.idx, -1, 0);
    if (!WRITE) cnt[q0] = rank;
}

// emission e of partition p (pbase[p] = rank of the partition's first emission) goes out in orientation
// m = start_marker toggled (e - pbase[p]) times
__device__ __forceinline__ int dyn_orientation(int64_t e, const uint64_t *pbase, int P, int start_marker) {
    int p = 0;
    for (int t = 1; t < P; t++) if ((int64_t)pbase[t] <= e) p = t;          // the last partition that starts at or before e
    const int64_t r = e - (int64_t)pbase[p];
    return (r & 1) ? 3 - start_marker : start_marker;
}

// what output record e is made of: key' = bases [kstart, kstart + klen) and ext' = bases [estart, estart + elen) of a
// concatenation.  singleKmerRandomizer (FirstFour:1857-1930) / reflexivExtend (:1957-2120):
//   flip 1 -> 2   key + ext:   key' = its last |key| bases, ext' = its first |ext|   (any lengths, as Iteration's array form;
//   flip 2 -> 1   ext + key:   key' = its first |key| bases, ext' = the rest          FirstFour's single-long form is the same
//   no flip, copy key + ext:   as they are                                            while |ext| <= |key|)
//   merge         P + L + S (reflected extension, the longer key, forward extension):
//                 m = 2: key' = the last |L| bases, ext' = the rest;  m = 1: key' = the first |L| bases, ext' = the rest
struct DynPlan { DynCat c; int kstart, klen, estart, elen; };
__device__ __forceinline__ const uint64_t *dyn_ext_ptr(const DynView &v, int64_t q) { return v.ext + v.ext_off[q]; }
__device__ __forceinline__ DynPlan dyn_plan(const DynView &v, const DynDesc d, int m) {
    DynPlan p;
    if (d.kind != 1) {
        const int kl = (int)v.key_len[d.a], el = v.ext_len[d.a], mk = v.marker[d.a];
        const uint64_t *K = v.key + DYN_KW * d.a, *E = dyn_ext_ptr(v, d.a);
        p.klen = kl; p.elen = el;
        p.c.w2 = nullptr; p.c.l2 = 0;
        if (d.kind == 0 && mk == 1 && m == 2) { p.c.w0 = K; p.c.l0 = kl; p.c.w1 = E; p.c.l1 = el; p.kstart = el; p.estart = 0; }
        else if (d.kind == 0 && mk == 2 && m == 1) { p.c.w0 = E; p.c.l0 = el; p.c.w1 = K; p.c.l1 = kl; p.kstart = 0; p.estart = kl; }
        else { p.c.w0 = K; p.c.l0 = kl; p.c.w1 = E; p.c.l1 = el; p.kstart = 0; p.estart = kl; }
        return p;
    }
    const int64_t f = d.a, r = d.b;
    const int kf = (int)v.key_len[f], kr = (int)v.key_len[r];
    const int S = v.ext_len[f], Pn = v.ext_len[r];
    const int Ln = kf >= kr ? kf : kr;
    p.c.w0 = dyn_ext_ptr(v, r); p.c.l0 = Pn;
    p.c.w1 = v.key + DYN_KW * (kf >= kr ? f : r); p.c.l1 = Ln;
    p.c.w2 = dyn_ext_ptr(v, f); p.c.l2 = S;
    p.klen = Ln; p.elen = Pn + S;
    if (m == 2) { p.kstart = Pn + S; p.estart = 0; } else { p.kstart = 0; p.estart = Ln; }
    return p;
}

// lengths, attributes and extension words of every emission (the bubble arithmetic of the merge is here)
__global__ __launch_bounds__(256) void k_dyn_sizes(const DynDesc *__restrict__ desc, int64_t ne, const DynView v, const uint64_t *__restrict__ pbase,
                                                   int P, int start_marker, const DynOut o, uint32_t *__restrict__ ew) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const DynDesc d = desc[e];
    const int m = d.kind == 2 ? 0 : dyn_orientation(e, pbase, P, start_marker);
    if (d.kind != 1) {
        const int kl = (int)v.key_len[d.a], el = v.ext_len[d.a], mk = v.marker[d.a];
        o.key_len[e] = (uint8_t)kl; o.ext_len[e] = el; ew[e] = (uint32_t)((el + 31) >> 5);
        o.left[e] = v.left[d.a]; o.right[e] = v.right[d.a];
        o.marker[e] = (d.kind == 0 && mk == 1 && m == 2) ? 2 : (d.kind == 0 && mk == 2 && m == 1) ? 1 : mk;
        return;
    }
    const int64_t f = d.a, r = d.b;
    const int kf = (int)v.key_len[f], kr = (int)v.key_len[r];
    const int S = v.ext_len[f], Pn = v.ext_len[r];
    const int extra = kf > kr ? kf - kr : 0;
    const int lf_f = v.left[f], lf_r = v.left[r], rt_f = v.right[f], rt_r = v.right[r];
    int lf, rt;
    if (d.bubble < 0) {
        lf = lf_r >= 0 ? lf_r : lf_f - Pn;
        rt = rt_f >= 0 ? rt_f : rt_r - S - extra;
    } else if (lf_f > 0) {
        lf = d.bubble;
        rt = rt_f >= 0 ? rt_f : rt_r - S - extra;
    } else {
        lf = lf_r >= 0 ? lf_r : lf_f - Pn;
        rt = d.bubble - extra;
    }
    o.left[e] = pk_clamp(lf); o.right[e] = pk_clamp(rt); o.marker[e] = m;
    o.key_len[e] = (uint8_t)(kf >= kr ? kf : kr);               // the longer key's length is kept
    o.ext_len[e] = Pn + S; ew[e] = (uint32_t)((Pn + S + 31) >> 5);
}
// one thread per output key word: all DYN_KW words of every record are written, the unused ones as 0
__global__ __launch_bounds__(256) void k_dyn_emit_key(const DynDesc *__restrict__ desc, int64_t ne, const DynView v, const uint64_t *__restrict__ pbase,
                                                      int P, int start_marker, uint64_t *__restrict__ okey) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ne * DYN_KW) return;
    const int64_t e = t / DYN_KW;
    const int j = (int)(t % DYN_KW);
    const DynDesc d = desc[e];
    const DynPlan p = dyn_plan(v, d, d.kind == 2 ? 0 : dyn_orientation(e, pbase, P, start_marker));
    okey[t] = pk_keep(dyn_cat32(p.c, p.kstart + 32 * j), p.klen - 32 * j);
}
// one thread per output extension word; its record through the scan of the word counts.  The grid covers the input's word
// bound; the exact total is oeoff[ne]
__global__ __launch_bounds__(256) void k_dyn_emit_ext(const DynDesc *__restrict__ desc, int64_t ne, const DynView v, const uint64_t *__restrict__ pbase,
                                                      int P, int start_marker, const int64_t *__restrict__ oeoff, uint64_t *__restrict__ oext) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ne <= 0 || w >= oeoff[ne]) return;
    const int64_t e = pk_find(oeoff, ne, w);
    const int j = (int)(w - oeoff[e]);
    const DynDesc d = desc[e];
    const DynPlan p = dyn_plan(v, d, d.kind == 2 ? 0 : dyn_orientation(e, pbase, P, start_marker));
    oext[w] = pk_keep(dyn_cat32(p.c, p.estart + 32 * j), p.elen - 32 * j);
}

// DSkmerRandomReflection.call (FirstFour:2518-2524): row q of partition p in orientation 2, 1, 2, ... by its rank
__global__ __launch_bounds__(256) void k_dyn_identity_desc(int64_t n, DynDesc *__restrict__ desc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) desc[i] = DynDesc{0, 0, i, -1};
}
// the gather behind the sort: output record i is a copy of record perm[i]
__global__ __launch_bounds__(256) void k_dyn_perm_desc(const uint32_t *__restrict__ perm, int64_t n, DynDesc *__restrict__ desc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) desc[i] = DynDesc{2, 0, (int64_t)perm[i], -1};
}
__global__ void k_dyn_copy_u64(const int64_t *__restrict__ src, int n, uint64_t *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (uint64_t)src[i];
}
// partition bases of the emissions: pbase[p] = base of the family that opens partition p (or the total)
__global__ void k_dyn_pbase(const int64_t *__restrict__ ps, int P, const uint64_t *__restrict__ base, int64_t n, uint64_t total,
                            uint64_t *__restrict__ pbase, int64_t *__restrict__ out_ps) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > P) return;
    const uint64_t v = (p == P || ps[p] >= n) ? total : base[ps[p]];
    pbase[p] = v;
    if (out_ps) out_ps[p] = (int64_t)v;
}

// descriptors -> the output record set; no host wait: the output is bounded by the input (ne <= in.n emissions of a pass,
// in.words extension words)
static int dyn_emit(rfx_ctx *ctx, const DynDev &in, const DevBuf &desc, int64_t ne, const uint64_t *d_pbase, int P, int start_marker, DynDev &out) {
    DevBuf ew;
    RFX_ALLOC(ew, uint32_t, std::max<int64_t>(ne, 1));
    RFX_TRY(dyn_alloc(ctx, out, ne, in.words));
    const DynView v = dyn_view(in);
    if (ne > 0) {
        RFX_LAUNCH_N(k_dyn_sizes, ne, desc.as<DynDesc>(), ne, v, d_pbase, P, start_marker, dyn_out(out), ew.as<uint32_t>());
    }
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, ew.as<uint32_t>(), out.ext_off.as<uint64_t>(), ne));
    if (ne > 0) {
        RFX_LAUNCH_N(k_dyn_emit_key, ne * DYN_KW, desc.as<DynDesc>(), ne, v, d_pbase, P, start_marker, out.key.as<uint64_t>());
        if (in.words > 0) {
            RFX_LAUNCH_N(k_dyn_emit_ext, in.words, desc.as<DynDesc>(), ne, v, d_pbase, P, start_marker,
                         out.ext_off.as<int64_t>(), out.ext.as<uint64_t>());
        }
    }
    return RFX_OK;
}

// the set's key lengths without a sort: too long -> RFX_E_LIMIT; *lmin = the shortest key (0 for an empty set)
static int dyn_check_lengths(rfx_ctx *ctx, const DynDev &in, uint32_t *lmin) {
    *lmin = 0;
    if (in.n == 0) return RFX_OK;
    DevBuf flags;
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_dyn_keys, in.n, in.key.as<uint64_t>(), in.key_len.as<uint8_t>(), in.n,
                 (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, flags.as<CallFlags>());
    CallFlags h{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &h));
    if (h.bad & DYN_TOO_LONG) { ctx->last_error = "dynamic-k: a key longer than 124 bases"; return RFX_E_LIMIT; }
    *lmin = h.min_len;
    return RFX_OK;
}

}  // namespace
// sort("k-1") + the cut into P logical partitions: in -> out (sorted), d_ps[P + 1]; *lmin = the shortest key
int rfx::dyn_sort(rfx_ctx *ctx, const DynDev &in, int P, DynDev &out, DevBuf &d_ps, uint32_t *lmin) {
    const int64_t n = in.n;
    RFX_TRY(part_starts_alloc(ctx, d_ps, P, n == 0));
    *lmin = 0;
    if (n == 0) return dyn_empty(ctx, out);
    if (n >= ((int64_t)1 << 32)) { ctx->last_error = "dynamic-k sort: more than 2^32 records"; return RFX_E_LIMIT; }
    DevBuf blk, nblk, perm, tk, tv, keys, flags, desc;
    RFX_ALLOC(blk, uint64_t, (size_t)DYN_MAXB * n); RFX_ALLOC(nblk, uint64_t, n);
    RFX_ALLOC(perm, uint32_t, n); RFX_ALLOC(tk, uint64_t, n); RFX_ALLOC(tv, uint32_t, n);
    RFX_ALLOC(keys, uint64_t, n);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_dyn_keys, n, in.key.as<uint64_t>(), in.key_len.as<uint8_t>(), n, blk.as<uint64_t>(),
                 nblk.as<uint64_t>(), perm.as<uint32_t>(), flags.as<CallFlags>());
    CallFlags h{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &h));
    if (h.bad & DYN_TOO_LONG) { ctx->last_error = "dynamic-k: a key longer than 124 bases"; return RFX_E_LIMIT; }
    *lmin = h.min_len;
    // LSD: the block count (a proper prefix first when every shared block is equal), then the blocks, last to first.  A block
    // no key of the set reaches is 0 for every record and a stable sort on it is the identity: skipped
    const int nb_max = h.max_len == 0 ? 1 : ((int)h.max_len - 1) / 31 + 1;
    for (int pass = -1; pass < nb_max; pass++) {
        const uint64_t *src = pass < 0 ? nblk.as<uint64_t>() : blk.as<uint64_t>() + (int64_t)(nb_max - 1 - pass) * n;
        if (pass < 0 && nb_max == 1) continue;                    // (every key has one block)
        RFX_LAUNCH_N(k_dyn_gather_u64, n, src, perm.as<uint32_t>(), n, keys.as<uint64_t>());
        RFX_TRY(sort_pairs(ctx, keys.as<uint64_t>(), perm.as<uint32_t>(), n, pass < 0 ? 8 : 64, tk.as<uint64_t>(), tv.as<uint32_t>()));
    }
    // gather the records through the permutation: the emission with "copy" descriptors
    RFX_ALLOC(desc, DynDesc, n);
    RFX_LAUNCH_N(k_dyn_perm_desc, n, perm.as<uint32_t>(), n, desc.as<DynDesc>());
    RFX_TRY(dyn_emit(ctx, in, desc, n, nullptr, P, 0, out));
    RFX_LAUNCH(k_dyn_part_starts, dim3(1), dim3(1), 0, out.key.as<uint64_t>(),
               out.key_len.as<uint8_t>(), n, P, d_ps.as<int64_t>());
    return RFX_OK;
}
namespace {
__global__ __launch_bounds__(256) void k_dyn_iota(uint32_t *__restrict__ perm, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (uint32_t)i;
}
}  // namespace
// a stable sort of n < 2^32 items by a key of W 64-bit words held as W columns of n entries (word j of item i = d_cols[j n + i], the
// most significant word first): d_perm[q] = the item at position q.  LSD over the columns, as dyn_sort runs over its blocks
int rfx::sort_columns(rfx_ctx *ctx, const uint64_t *d_cols, int W, int64_t n, uint32_t *d_perm) {
    if (n == 0) return RFX_OK;
    DevBuf tk, tv, keys;
    RFX_ALLOC(tk, uint64_t, n); RFX_ALLOC(tv, uint32_t, n); RFX_ALLOC(keys, uint64_t, n);
    RFX_LAUNCH_N(k_dyn_iota, n, d_perm, n);
    for (int j = W - 1; j >= 0; j--) {
        RFX_LAUNCH_N(k_dyn_gather_u64, n, d_cols + (int64_t)j * n, d_perm, n, keys.as<uint64_t>());
        RFX_TRY(sort_pairs(ctx, keys.as<uint64_t>(), d_perm, n, 64, tk.as<uint64_t>(), tv.as<uint32_t>()));
    }
    return sync_checked(ctx);                                     // (the scratch above is read until here)
}
// one pass over sorted records: in (sorted), d_ps -> out, d_out_ps (optional)
int rfx::dyn_pass(rfx_ctx *ctx, const DynDev &in, const int64_t *d_ps, int P, uint32_t lmin, int stage, int start_iteration, int start_marker,
                  DynDev &out, int64_t *d_out_ps) {
    const int64_t n = in.n;
    DevBuf head, cnt, base, desc, pbase;
    RFX_ALLOC(pbase, uint64_t, P + 1);
    if (n == 0) {
        RFX_HIP(hipMemsetAsync(pbase.p, 0, (size_t)(P + 1) * 8, ctx->stream));
        if (d_out_ps) RFX_HIP(hipMemsetAsync(d_out_ps, 0, (size_t)(P + 1) * 8, ctx->stream));
        RFX_HIP(desc.alloc(sizeof(DynDesc), ctx->stream));
        return dyn_emit(ctx, in, desc, 0, pbase.as<uint64_t>(), P, start_marker, out);
    }
    RFX_ALLOC(head, uint32_t, n); RFX_ALLOC(cnt, uint32_t, n); RFX_ALLOC(base, uint64_t, n + 1);
    RFX_ALLOC(desc, DynDesc, n);
    const DynView v = dyn_view(in);
    RFX_LAUNCH_N(k_dyn_heads, n, v.key, n, d_ps, P, lmin, head.as<uint32_t>());
    RFX_LAUNCH(k_dyn_walk<false>, dim3((unsigned)ceil_div(n, 128)), dim3(128), 0, v, n, head.as<uint32_t>(), stage,
               start_iteration, cnt.as<uint32_t>(), (const uint64_t *)nullptr, (DynDesc *)nullptr);
    int64_t ne = 0;
    RFX_TRY(scan_keep(ctx, cnt.as<uint32_t>(), n, base.as<uint64_t>(), &ne));
    RFX_LAUNCH(k_dyn_walk<true>, dim3((unsigned)ceil_div(n, 128)), dim3(128), 0, v, n, head.as<uint32_t>(), stage,
               start_iteration, (uint32_t *)nullptr, base.as<uint64_t>(), desc.as<DynDesc>());
    RFX_LAUNCH(k_dyn_pbase, dim3(1), dim3(64), 0, d_ps, P, base.as<uint64_t>(), n, (uint64_t)ne, pbase.as<uint64_t>(), d_out_ps);
    return dyn_emit(ctx, in, desc, ne, pbase.as<uint64_t>(), P, start_marker, out);
}
namespace {

static int dyn_reflect(rfx_ctx *ctx, const DynDev &in, const int64_t *d_ps, int P, DynDev &out) {
    DevBuf desc, pbase;
    RFX_ALLOC(desc, DynDesc, std::max<int64_t>(in.n, 1));
    RFX_ALLOC(pbase, uint64_t, P + 1);
    RFX_LAUNCH_N(k_dyn_identity_desc, in.n, in.n, desc.as<DynDesc>());
    RFX_LAUNCH(k_dyn_copy_u64, dim3(1), dim3(64), 0, d_ps, P + 1, pbase.as<uint64_t>());
    return dyn_emit(ctx, in, desc, in.n, pbase.as<uint64_t>(), P, 2, out);
}

// ---- host base codes <-> the packed set ---------------------------------------------------------------------------------------
// sizes: key_len / ext_len / extension words of every record from the host form's offsets
__global__ __launch_bounds__(256) void k_dyn_pack_sizes(const int64_t *__restrict__ koff, const int64_t *__restrict__ eoff, int64_t n,
                                                        uint8_t *__restrict__ key_len, int32_t *__restrict__ ext_len, uint32_t *__restrict__ ew,
                                                        CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    int64_t kl = live ? koff[i + 1] - koff[i] : 0, el = live ? eoff[i + 1] - eoff[i] : 0;
    if (live && (kl < 0 || el < 0 || el > 0x7FFFFFE0ll)) { atomicOr(&flags->bad, (uint32_t)DYN_BAD_OFFSETS); kl = kl < 0 ? 0 : kl; el = 0; }
    dyn_note_lengths(flags, live, (int)(kl > 255 ? 255 : kl));
    if (!live) return;
    key_len[i] = (uint8_t)(kl > 255 ? 255 : kl);
    ext_len[i] = (int32_t)el;
    ew[i] = (uint32_t)((el + 31) >> 5);
}
// 32 base codes (one byte each) -> one word, the first in the two highest bits; cnt < 32: the rest 0
__device__ __forceinline__ uint64_t dyn_pack32(const uint8_t *__restrict__ s, int cnt) {
    uint64_t x = 0;
    for (int i = 0; i < 32; i++) if (i < cnt) x |= (uint64_t)(s[i] & 3) << (62 - 2 * i);
    return x;
}
__global__ __launch_bounds__(256) void k_dyn_pack_key(const uint8_t *__restrict__ key, const int64_t *__restrict__ koff, const uint8_t *__restrict__ key_len,
                                                      int64_t n, uint64_t *__restrict__ okey) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * DYN_KW) return;
    const int64_t i = t / DYN_KW;
    const int j = (int)(t % DYN_KW);
    const int cnt = (int)key_len[i] - 32 * j;
    okey[t] = cnt > 0 ? dyn_pack32(key + koff[i] + 32 * j, cnt) : 0ull;
}
__global__ __launch_bounds__(256) void k_dyn_pack_ext(const uint8_t *__restrict__ ext, const int64_t *__restrict__ eoff, const int32_t *__restrict__ ext_len,
                                                      int64_t n, const int64_t *__restrict__ oeoff, uint64_t *__restrict__ oext) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n <= 0 || w >= oeoff[n]) return;
    const int64_t i = pk_find(oeoff, n, w);
    const int j = (int)(w - oeoff[i]);
    oext[w] = dyn_pack32(ext + eoff[i] + 32 * (int64_t)j, ext_len[i] - 32 * j);
}

// host record set -> a packed set in HBM (the library's own buffers).  A key of more than 124 bases: RFX_E_LIMIT
static int dyn_pack_host(rfx_ctx *ctx, const rfx_dyn_records *h, DynDev &d) {
    const int64_t n = h->n;
    if (n < 0 || (n > 0 && (!h->key_off || !h->ext_off || !h->marker || !h->left || !h->right))) return RFX_E_ARG;
    const int64_t nk = n ? h->key_off[n] : 0, ne = n ? h->ext_off[n] : 0;
    if (nk < 0 || ne < 0 || (nk > 0 && !h->key) || (ne > 0 && !h->ext)) return RFX_E_ARG;
    RFX_TRY(dyn_alloc(ctx, d, n, n + ne / 32));
    if (n == 0) {
        RFX_HIP(hipMemsetAsync(d.ext_off.p, 0, 8, ctx->stream));
        return RFX_OK;
    }
    DevBuf kb, eb, ko, eo, ew, flags;
    RFX_HIP(kb.alloc((size_t)std::max<int64_t>(nk, 1), ctx->stream)); RFX_HIP(eb.alloc((size_t)std::max<int64_t>(ne, 1), ctx->stream));
    RFX_ALLOC(ko, int64_t, n + 1); RFX_ALLOC(eo, int64_t, n + 1);
    RFX_ALLOC(ew, uint32_t, n);
    RFX_TRY(call_flags_init(ctx, flags));
    if (nk) RFX_HIP(hipMemcpyAsync(kb.p, h->key, (size_t)nk, hipMemcpyHostToDevice, ctx->stream));
    if (ne) RFX_HIP(hipMemcpyAsync(eb.p, h->ext, (size_t)ne, hipMemcpyHostToDevice, ctx->stream));
    RFX_HIP(hipMemcpyAsync(ko.p, h->key_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    RFX_HIP(hipMemcpyAsync(eo.p, h->ext_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    RFX_HIP(hipMemcpyAsync(d.marker.p, h->marker, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    RFX_HIP(hipMemcpyAsync(d.left.p, h->left, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    RFX_HIP(hipMemcpyAsync(d.right.p, h->right, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    RFX_LAUNCH_N(k_dyn_pack_sizes, n, ko.as<int64_t>(), eo.as<int64_t>(), n, d.key_len.as<uint8_t>(),
                 d.ext_len.as<int32_t>(), ew.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, ew.as<uint32_t>(), d.ext_off.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));
    if (f.bad & DYN_BAD_OFFSETS) { ctx->last_error = "dynamic-k: record offsets that run backwards"; return RFX_E_ARG; }
    if (f.bad & DYN_TOO_LONG) { ctx->last_error = "dynamic-k: a key longer than 124 bases"; return RFX_E_LIMIT; }
    RFX_LAUNCH_N(k_dyn_pack_key, n * DYN_KW, kb.as<uint8_t>(), ko.as<int64_t>(),
                 d.key_len.as<uint8_t>(), n, d.key.as<uint64_t>());
    if (d.words > 0) {
        RFX_LAUNCH_N(k_dyn_pack_ext, d.words, eb.as<uint8_t>(), eo.as<int64_t>(),
                     d.ext_len.as<int32_t>(), n, d.ext_off.as<int64_t>(), d.ext.as<uint64_t>());
    }
    return sync_checked(ctx);                                     // (the staging buffers are read by the copies queued above)
}

__global__ __launch_bounds__(256) void k_dyn_unpack_sizes(const uint8_t *__restrict__ key_len, const int32_t *__restrict__ ext_len, int64_t n,
                                                          uint32_t *__restrict__ ks, uint32_t *__restrict__ es) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ks[i] = (uint32_t)key_len[i];
    es[i] = (uint32_t)ext_len[i];
}
// one thread per output base: its record through the scan of the lengths.  word_off == nullptr: DYN_KW words per record
__global__ __launch_bounds__(256) void k_dyn_unpack_bases(const uint64_t *__restrict__ words, const int64_t *__restrict__ word_off, const uint64_t *__restrict__ boff,
                                                          int64_t n, int64_t total, uint8_t *__restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= total) return;
    const int64_t i = pk_find(boff, n, b);
    const int64_t t = b - (int64_t)boff[i];
    const uint64_t *w = words + (word_off ? word_off[i] : DYN_KW * i);
    out[b] = (uint8_t)((w[t >> 5] >> (62 - 2 * (int)(t & 31))) & 3);
}

// a packed set -> the caller's host arrays; checks every capacity before anything is copied
static int dyn_unpack_host(rfx_ctx *ctx, const DynDev &d, rfx_dyn_records *h) {
    const int64_t n = d.n;
    DevBuf ks, es, kso, eso, kb, eb;
    RFX_ALLOC(ks, uint32_t, std::max<int64_t>(n, 1)); RFX_ALLOC(es, uint32_t, std::max<int64_t>(n, 1));
    RFX_ALLOC(kso, uint64_t, n + 1); RFX_ALLOC(eso, uint64_t, n + 1);
    if (n > 0) {
        RFX_LAUNCH_N(k_dyn_unpack_sizes, n, d.key_len.as<uint8_t>(), d.ext_len.as<int32_t>(), n,
                     ks.as<uint32_t>(), es.as<uint32_t>());
    }
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, ks.as<uint32_t>(), es.as<uint32_t>(), kso.as<uint64_t>(), eso.as<uint64_t>(), n));
    uint64_t tot[2] = {0, 0};
    RFX_HIP(hipMemcpyAsync(&tot[0], kso.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_HIP(hipMemcpyAsync(&tot[1], eso.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_TRY(sync_checked(ctx));
    const int64_t nk = (int64_t)tot[0], ne = (int64_t)tot[1];
    h->n = n; h->need_key = nk; h->need_ext = ne;
    if (n > h->cap_n || nk > h->cap_key || ne > h->cap_ext) return RFX_E_CAP;
    RFX_HIP(kb.alloc((size_t)std::max<int64_t>(nk, 1), ctx->stream)); RFX_HIP(eb.alloc((size_t)std::max<int64_t>(ne, 1), ctx->stream));
    if (nk) {
        RFX_LAUNCH_N(k_dyn_unpack_bases, nk, d.key.as<uint64_t>(), (const int64_t *)nullptr, kso.as<uint64_t>(),
                     n, nk, kb.as<uint8_t>());
        RFX_HIP(hipMemcpyAsync(h->key, kb.p, (size_t)nk, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (ne) {
        RFX_LAUNCH_N(k_dyn_unpack_bases, ne, d.ext.as<uint64_t>(), d.ext_off.as<int64_t>(),
                     eso.as<uint64_t>(), n, ne, eb.as<uint8_t>());
        RFX_HIP(hipMemcpyAsync(h->ext, eb.p, (size_t)ne, hipMemcpyDeviceToHost, ctx->stream));
    }
    RFX_HIP(hipMemcpyAsync(h->key_off, kso.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_HIP(hipMemcpyAsync(h->ext_off, eso.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n) {
        RFX_HIP(hipMemcpyAsync(h->marker, d.marker.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RFX_HIP(hipMemcpyAsync(h->left, d.left.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RFX_HIP(hipMemcpyAsync(h->right, d.right.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    return sync_checked(ctx);
}

}  // namespace
// ---- what every stage on packed sets shares (rfx_internal.h): the host checks, the empty set, the flags of a call ------------------
bool rfx::dyn_packed_out_ok(const rfx_dyn_packed *p) {
    return p && p->key && p->key_len && p->ext && p->ext_off && p->ext_len && p->marker && p->left && p->right;
}
bool rfx::dyn_packed_ok(const rfx_dyn_packed *p) { return dyn_packed_out_ok(p) && p->n >= 0; }
bool rfx::text_rows_ok(const char *text, const int64_t *row_off, int64_t n) { return n >= 0 && (n == 0 || (text && row_off)); }
int rfx::dyn_empty(rfx_ctx *ctx, DynDev &d) {
    RFX_TRY(dyn_alloc(ctx, d, 0, 0));
    RFX_HIP(hipMemsetAsync(d.ext_off.p, 0, 8, ctx->stream));
    return RFX_OK;
}
bool rfx::parts_ok(int P) { return P >= 1 && P <= 63; }
int rfx::check_part_starts(rfx_ctx *ctx, const int64_t *d_ps, int P, int64_t n, const char *stage_name) {
    int64_t h[65];
    RFX_TRY(small_readback(ctx, h, d_ps, (size_t)(P + 1) * 8));
    bool ok = h[0] == 0 && h[P] == n;
    for (int p = 0; p < P && ok; p++) ok = h[p] <= h[p + 1];
    if (!ok) { ctx->last_error = std::string(stage_name) + ": partition starts that do not run from 0 to n"; return RFX_E_ARG; }
    return RFX_OK;
}
int rfx::call_flags_init(rfx_ctx *ctx, DevBuf &flags) {
    RFX_HIP(flags.alloc(sizeof(CallFlags), ctx->stream));
    RFX_HIP(hipMemsetAsync(flags.p, 0, sizeof(CallFlags), ctx->stream));
    RFX_HIP(hipMemsetAsync(&flags.as<CallFlags>()->min_len, 0xFF, 4, ctx->stream));
    return RFX_OK;
}
namespace {
__global__ void k_put_totals(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, const uint64_t *__restrict__ c, CallFlags *__restrict__ flags) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { flags->total[0] = a ? *a : 0ull; flags->total[1] = b ? *b : 0ull; flags->total[2] = c ? *c : 0ull; }
}
}  // namespace
int rfx::call_flags_read(rfx_ctx *ctx, const DevBuf &flags, const uint64_t *d_t0, const uint64_t *d_t1, const uint64_t *d_t2, CallFlags *h) {
    if (d_t0 || d_t1 || d_t2) RFX_LAUNCH(k_put_totals, dim3(1), dim3(1), 0, d_t0, d_t1, d_t2, flags.as<CallFlags>());
    return small_readback(ctx, h, flags.p, sizeof(CallFlags));
}
// ---- the host steps the stages share (rfx_internal.h) -----------------------------------------------------------------------------
namespace {
__global__ void k_out_part_starts(const int64_t *__restrict__ ps, int P, const uint64_t *__restrict__ off, int64_t *__restrict__ out_ps) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p <= P) out_ps[p] = (int64_t)off[ps[p]];
}
__global__ __launch_bounds__(256) void k_index_kept(const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank, int64_t n, int64_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && keep[i]) idx[rank[i]] = i;
}
}  // namespace
int rfx::scan_keep(rfx_ctx *ctx, const uint32_t *d_keep, int64_t n, uint64_t *d_rank, int64_t *total) {
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, d_keep, d_rank, n));
    uint64_t t = 0;
    RFX_TRY(small_readback(ctx, &t, d_rank + n, 8));
    *total = (int64_t)t;
    return RFX_OK;
}
int rfx::part_starts_alloc(rfx_ctx *ctx, DevBuf &out_ps, int P, bool zeroed) {
    RFX_ALLOC(out_ps, int64_t, P + 1);
    if (zeroed) RFX_HIP(hipMemsetAsync(out_ps.p, 0, (size_t)(P + 1) * sizeof(int64_t), ctx->stream));
    return RFX_OK;
}
int rfx::part_starts_store(rfx_ctx *ctx, int64_t *d_dst, const DevBuf &ops, int P) {
    RFX_HIP(hipMemcpyAsync(d_dst, ops.p, (size_t)(P + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
    return sync_checked(ctx);
}
int rfx::out_part_starts(rfx_ctx *ctx, const int64_t *d_ps, int P, const uint64_t *d_prefix, int64_t *d_out) {
    RFX_LAUNCH(k_out_part_starts, dim3(1), dim3(64), 0, d_ps, P, d_prefix, d_out);
    return RFX_OK;
}
int rfx::index_kept(rfx_ctx *ctx, const uint32_t *d_keep, const uint64_t *d_rank, int64_t n, int64_t *d_idx) {
    RFX_LAUNCH_N(k_index_kept, n, d_keep, d_rank, n, d_idx);
    return RFX_OK;
}
int rfx::text_to_host(rfx_ctx *ctx, std::initializer_list<TextOut> outs, bool fill_to_cap) {
    bool too_short = false;
    for (const TextOut &o : outs) { *o.out_len = o.total; too_short |= o.total > o.cap; }
    if (too_short && !fill_to_cap) return RFX_E_CAP;
    for (const TextOut &o : outs) {
        const int64_t lim = std::min<int64_t>(o.total, o.cap);
        if (lim > 0) RFX_HIP(hipMemcpyAsync(o.out, o.d.p, (size_t)lim, hipMemcpyDeviceToHost, ctx->stream));
    }
    RFX_TRY(sync_checked(ctx));
    return too_short ? RFX_E_CAP : RFX_OK;
}
// ---- the caller's packed arrays (rfx_dyn_packed, device pointers) <-> DynDev ---------------------------------------------------
// a view of the caller's input set: nothing is copied, nothing is freed
int rfx::dyn_borrow(rfx_ctx *ctx, const rfx_dyn_packed *p, DynDev &d) {
    auto b = [&](DevBuf &x, void *q) { x.release(); x.p = q; x.s = ctx->stream; x.borrowed = true; };
    b(d.key, p->key); b(d.key_len, p->key_len); b(d.ext, p->ext); b(d.ext_off, p->ext_off); b(d.ext_len, p->ext_len);
    b(d.marker, p->marker); b(d.left, p->left); b(d.right, p->right);
    d.n = p->n; d.words = 0;
    if (p->n > 0) {
        int64_t w = 0;
        RFX_TRY(small_readback(ctx, &w, p->ext_off + p->n, 8));
        if (w < 0) return RFX_E_ARG;
        d.words = w;
    }
    return RFX_OK;
}
// the result into the caller's arrays; checks both capacities before anything is copied
int rfx::dyn_store(rfx_ctx *ctx, const DynDev &d, rfx_dyn_packed *o) {
    const int64_t n = d.n;
    int64_t words = 0;
    if (n > 0) RFX_TRY(small_readback(ctx, &words, d.ext_off.as<int64_t>() + n, 8));
    o->n = n; o->need_words = words;
    if (n > o->cap_n || words > o->cap_words) return RFX_E_CAP;
    if (n > 0) {
        RFX_HIP(hipMemcpyAsync(o->key, d.key.p, (size_t)n * DYN_KW * 8, hipMemcpyDeviceToDevice, ctx->stream));
        RFX_HIP(hipMemcpyAsync(o->key_len, d.key_len.p, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        if (words) RFX_HIP(hipMemcpyAsync(o->ext, d.ext.p, (size_t)words * 8, hipMemcpyDeviceToDevice, ctx->stream));
        RFX_HIP(hipMemcpyAsync(o->ext_off, d.ext_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
        RFX_HIP(hipMemcpyAsync(o->ext_len, d.ext_len.p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        RFX_HIP(hipMemcpyAsync(o->marker, d.marker.p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        RFX_HIP(hipMemcpyAsync(o->left, d.left.p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        RFX_HIP(hipMemcpyAsync(o->right, d.right.p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        RFX_HIP(hipMemsetAsync(o->ext_off, 0, 8, ctx->stream));
    }
    return sync_checked(ctx);
}
namespace {

// ---- DynamicKmerBinarizerFromReducedToSubKmer (FirstFour :2931-3016; Iteration's twin) on the device: the text rows of the hand-over
// files -> records.  A row is its fields joined by ',': form 0 = (k-mer, "m|l|r") -- key = the k-mer without its last base, extension =
// that base, orientation 1 --, form 1 = (sub-k-mer, "m|l|r", extension).  A leading '(' of the first field and a trailing ')' of the
// attribute are dropped (the tuple text Spark writes); left / right are read back clamped to +-30000 (buildingAlongFromThreeInt
// :2340-2366); A0 C1 G2, anything else 3.  Sizes (one thread per row: the cut, the attribute, where key and extension begin in the
// text), a scan of the extension words, then the fill: one thread per output word packs its 32 letters.
struct DynRowCut { int64_t f0, f0e, f1, f1e, f2, f2e; };     // the three fields' [begin, end) in the text
__device__ __forceinline__ DynRowCut dyn_row_cut(const char *__restrict__ t, int64_t b, int64_t e) {
    while (e > b && (t[e - 1] == '\n' || t[e - 1] == '\r')) e--;
    int64_t c1 = e, c2 = e;
    for (int64_t i = b; i < e; i++) if (t[i] == ',') { if (c1 == e) c1 = i; else { c2 = i; break; } }
    DynRowCut c{b, c1, c1 < e ? c1 + 1 : e, c2, c2 < e ? c2 + 1 : e, e};
    if (c.f0 < c.f0e && t[c.f0] == '(') c.f0++;
    if (c.f1e > c.f1 && t[c.f1e - 1] == ')') c.f1e--;
    if (c.f2e > c.f2 && t[c.f2e - 1] == ')') c.f2e--;
    return c;
}
__global__ __launch_bounds__(256) void k_dyn_bin_sizes(const char *__restrict__ text, const int64_t *__restrict__ row_off, int64_t n, int form,
                                                       const DynOut o, int64_t *__restrict__ kbeg, int64_t *__restrict__ ebeg, uint32_t *__restrict__ ew,
                                                       CallFlags *__restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = r < n;
    int64_t kl = 0, el = 0;
    if (live) {
        int64_t b = row_off[r], e = row_off[r + 1];
        if (e < b) { atomicOr(&flags->bad, (uint32_t)DYN_BAD_OFFSETS); e = b; }
        const DynRowCut c = dyn_row_cut(text, b, e);
        const int64_t l0 = c.f0e - c.f0;
        if (form == 0) { kl = l0 > 0 ? l0 - 1 : 0; el = l0 > 0 ? 1 : 0; ebeg[r] = c.f0 + kl; }
        else { kl = l0; el = c.f2e - c.f2; ebeg[r] = c.f2; }
        if (el > 0x7FFFFFE0ll) { atomicOr(&flags->bad, (uint32_t)DYN_BAD_OFFSETS); el = 0; }
        kbeg[r] = c.f0;
        int64_t i = c.f1;
        const int m = pk_parse_int(text, i, c.f1e), l = pk_parse_int(text, i, c.f1e), rr = pk_parse_int(text, i, c.f1e);
        o.marker[r] = form == 0 ? 1 : m;
        o.left[r] = pk_clamp(l);
        o.right[r] = pk_clamp(rr);
        o.key_len[r] = (uint8_t)(kl > 255 ? 255 : kl);
        o.ext_len[r] = (int32_t)el;
        ew[r] = (uint32_t)((el + 31) >> 5);
    }
    dyn_note_lengths(flags, live, (int)(kl > 255 ? 255 : kl));
}
__device__ __forceinline__ uint64_t dyn_code32(const char *__restrict__ s, int cnt) {
    uint64_t x = 0;
    for (int i = 0; i < 32; i++) if (i < cnt) { const char ch = s[i]; x |= pk_code(ch) << (62 - 2 * i); }
    return x;
}
__global__ __launch_bounds__(256) void k_dyn_bin_key(const char *__restrict__ text, const int64_t *__restrict__ kbeg, const uint8_t *__restrict__ key_len,
                                                     int64_t n, uint64_t *__restrict__ okey) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * DYN_KW) return;
    const int64_t r = t / DYN_KW;
    const int j = (int)(t % DYN_KW);
    const int cnt = (int)key_len[r] - 32 * j;
    okey[t] = cnt > 0 ? dyn_code32(text + kbeg[r] + 32 * j, cnt) : 0ull;
}
__global__ __launch_bounds__(256) void k_dyn_bin_ext(const char *__restrict__ text, const int64_t *__restrict__ ebeg, const int32_t *__restrict__ ext_len,
                                                     int64_t n, const int64_t *__restrict__ oeoff, uint64_t *__restrict__ oext) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n <= 0 || w >= oeoff[n]) return;
    const int64_t r = pk_find(oeoff, n, w);
    const int j = (int)(w - oeoff[r]);
    oext[w] = dyn_code32(text + ebeg[r] + 32 * (int64_t)j, ext_len[r] - 32 * j);
}

}  // namespace
// text in HBM (row r = d_text[d_row_off[r], d_row_off[r + 1])) -> a packed set in the library's own buffers
int rfx::dyn_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, int form, DynDev &d) {
    if (n == 0) return dyn_empty(ctx, d);
    DevBuf kbeg, ebeg, ew, flags;
    const size_t m = (size_t)n;
    // (everything but the extension words, whose number the scan gives)
    RFX_ALLOC(d.key, uint64_t, m * DYN_KW); RFX_HIP(d.key_len.alloc(m, ctx->stream)); RFX_ALLOC(d.ext_off, uint64_t, m + 1);
    RFX_ALLOC(d.ext_len, int32_t, m); RFX_ALLOC(d.marker, int32_t, m); RFX_ALLOC(d.left, int32_t, m);
    RFX_ALLOC(d.right, int32_t, m);
    RFX_ALLOC(kbeg, int64_t, m); RFX_ALLOC(ebeg, int64_t, m); RFX_ALLOC(ew, uint32_t, m);
    RFX_TRY(call_flags_init(ctx, flags));
    d.n = n;
    RFX_LAUNCH_N(k_dyn_bin_sizes, n, d_text, d_row_off, n, form, dyn_out(d), kbeg.as<int64_t>(), ebeg.as<int64_t>(), ew.as<uint32_t>(),
                 flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, ew.as<uint32_t>(), d.ext_off.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, d.ext_off.as<uint64_t>() + n, nullptr, nullptr, &f));
    if (f.bad & DYN_BAD_OFFSETS) { ctx->last_error = "dynamic-k binarizer: row offsets that run backwards"; return RFX_E_ARG; }
    if (f.bad & DYN_TOO_LONG) { ctx->last_error = "dynamic-k: a key longer than 124 bases"; return RFX_E_LIMIT; }
    d.words = (int64_t)f.total[0];
    RFX_ALLOC(d.ext, uint64_t, std::max<int64_t>(d.words, 1));
    RFX_LAUNCH_N(k_dyn_bin_key, n * DYN_KW, d_text, kbeg.as<int64_t>(), d.key_len.as<uint8_t>(), n,
                 d.key.as<uint64_t>());
    if (d.words > 0) {
        RFX_LAUNCH_N(k_dyn_bin_ext, d.words, d_text, ebeg.as<int64_t>(), d.ext_len.as<int32_t>(), n,
                     d.ext_off.as<int64_t>(), d.ext.as<uint64_t>());
    }
    return RFX_OK;
}
// host text -> HBM: the rows' bytes and their offsets relative to the first row
int rfx::dyn_upload_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, DevBuf &d_text, DevBuf &d_off) {
    for (int64_t i = 0; i < n_rows; i++) if (row_off[i + 1] < row_off[i]) return RFX_E_ARG;
    const int64_t nb = n_rows ? row_off[n_rows] - row_off[0] : 0;
    RFX_HIP(d_text.alloc((size_t)std::max<int64_t>(nb, 1), ctx->stream));
    RFX_ALLOC(d_off, int64_t, n_rows + 1);
    if (n_rows == 0) return RFX_OK;
    std::vector<int64_t> rel((size_t)n_rows + 1);
    for (int64_t i = 0; i <= n_rows; i++) rel[(size_t)i] = row_off[i] - row_off[0];
    if (nb) RFX_HIP(hipMemcpyAsync(d_text.p, text + row_off[0], (size_t)nb, hipMemcpyHostToDevice, ctx->stream));
    RFX_HIP(hipMemcpyAsync(d_off.p, rel.data(), (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    return sync_checked(ctx);                                     // (rel is read by the copy)
}
namespace {

// ---- DSBinarySubKmerWith{Short,Long}ExtensionToString (FirstFour:226-263): rows "SUBKMER,marker|left|right,EXTENSION\n" ----------
__global__ __launch_bounds__(256) void k_dyn_text_sizes(const DynView v, int64_t n, uint64_t *__restrict__ sz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sz[i] = (uint64_t)v.key_len[i] + (uint64_t)v.ext_len[i] + 5 + pk_int_chars(v.marker[i]) + pk_int_chars(v.left[i]) + pk_int_chars(v.right[i]);
}
// one thread per output byte, up to lim (the smaller of the text's length and the buffer)
__global__ __launch_bounds__(256) void k_dyn_text_fill(const DynView v, int64_t n, const uint64_t *__restrict__ toff, int64_t lim, char *__restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= lim) return;
    const int64_t i = pk_find(toff, n, b);
    int64_t q = b - (int64_t)toff[i];
    const int kl = (int)v.key_len[i], el = v.ext_len[i];
    char ch;
    if (q < kl) ch = (char)pk_letter(pk_base_of(v.key + DYN_KW * i, (int)q));
    else {
        q -= kl;
        const int m = v.marker[i], l = v.left[i], r = v.right[i];
        const int cm = pk_int_chars(m), cl = pk_int_chars(l), cr = pk_int_chars(r);
        if (q == 0) ch = ',';
        else if (q < 1 + cm) ch = pk_int_char(m, (int)q - 1);
        else if (q == 1 + cm) ch = '|';
        else if (q < 2 + cm + cl) ch = pk_int_char(l, (int)q - 2 - cm);
        else if (q == 2 + cm + cl) ch = '|';
        else if (q < 3 + cm + cl + cr) ch = pk_int_char(r, (int)q - 3 - cm - cl);
        else if (q == 3 + cm + cl + cr) ch = ',';
        else {
            q -= 4 + cm + cl + cr;
            ch = q < el ? (char)pk_letter(pk_base_of(v.ext + v.ext_off[i], (int)q)) : '\n';
        }
    }
    out[b] = ch;
}
}  // namespace
// the text of a set into d_text (filled up to cap); *total = its length
int rfx::dyn_to_text(rfx_ctx *ctx, const DynDev &d, char *d_text, int64_t cap, int64_t *total, DevBuf *own) {
    const int64_t n = d.n;
    *total = 0;
    if (n == 0) return RFX_OK;
    DevBuf sz, toff;
    RFX_ALLOC(sz, uint64_t, n); RFX_ALLOC(toff, uint64_t, n + 1);
    const DynView v = dyn_view(d);
    RFX_LAUNCH_N(k_dyn_text_sizes, n, v, n, sz.as<uint64_t>());
    RFX_TRY(exclusive_scan_u64(ctx, sz.as<uint64_t>(), toff.as<uint64_t>(), n));
    uint64_t t = 0;
    RFX_TRY(small_readback(ctx, &t, toff.as<uint64_t>() + n, 8));
    *total = (int64_t)t;
    if (own) {                                                    // (the driver: a buffer of the library's, as long as the text)
        RFX_HIP(own->alloc((size_t)std::max<int64_t>(*total, 1), ctx->stream));
        d_text = own->as<char>(); cap = *total;
    }
    const int64_t lim = std::min<int64_t>(*total, cap);
    if (lim > 0) {
        RFX_LAUNCH_N(k_dyn_text_fill, lim, v, n, toff.as<uint64_t>(), lim, d_text);
    }
    return sync_checked(ctx);
}
namespace {

// The drivers, records resident in HBM between the operators.  FirstFour.assemblyFromKmer (:137-224): binarized records
// (key = the k-mer without its last base, extension = that base, orientation 1) -> DSkmerRandomReflection on P equal
// shares -> 4 x (sort, DSExtendReflexivKmer).  Iteration.assemblyFromKmer (:134-205): (end - start + 1) x (sort,
// DSExtendReflexivKmerToArrayLoop).  passes_first_four / start / end select what runs; a = the set, replaced by the result.
static int dyn_run(rfx_ctx *ctx, DynDev &a, int P, int random_reflection, int passes_first_four, int start_iteration, int end_iteration,
                   int64_t *trace, int64_t trace_cap, int64_t *n_trace) {
    DevBuf ps;
    int64_t nt = 0;
    if (random_reflection) {
        std::vector<int64_t> st((size_t)P + 1);
        for (int p = 0; p <= P; p++) st[(size_t)p] = p == P ? a.n : (int64_t)(((__int128)p * (__int128)a.n) / P);
        RFX_ALLOC(ps, int64_t, P + 1);
        RFX_HIP(hipMemcpyAsync(ps.p, st.data(), (size_t)(P + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        RFX_TRY(sync_checked(ctx));
        DynDev b;
        RFX_TRY(dyn_reflect(ctx, a, ps.as<int64_t>(), P, b));
        std::swap(a, b);
    }
    auto one = [&](int stage, int start_it) -> int {
        uint32_t lmin = 0;
        DynDev s;
        RFX_TRY(dyn_sort(ctx, a, P, s, ps, &lmin));
        DynDev o;
        RFX_TRY(dyn_pass(ctx, s, ps.as<int64_t>(), P, lmin, stage, start_it, 2, o, nullptr));
        RFX_TRY(sync_checked(ctx));
        std::swap(a, o);
        if (trace && nt < trace_cap) trace[nt] = a.n;
        nt++;
        return RFX_OK;
    };
    for (int i = 0; i < passes_first_four; i++) RFX_TRY(one(0, 0));
    for (int it = start_iteration; end_iteration >= start_iteration && it <= end_iteration; it++) RFX_TRY(one(1, start_iteration));
    if (n_trace) *n_trace = nt;
    return RFX_OK;
}

}  // namespace
// ... for the driver from reads to contigs (rfx_meta.hip): the body of rfx_dev_dyn_run on a set of the library's, replaced by the result
int rfx::dyn_run_set(rfx_ctx *ctx, DynDev &a, int P, int random_reflection, int passes_first_four, int start_iteration, int end_iteration) {
    return dyn_run(ctx, a, P, random_reflection, passes_first_four, start_iteration, end_iteration, nullptr, 0, nullptr);
}

extern "C" {

// ---- the packed set in the caller's device arrays ------------------------------------------------------------------------------
int rfx_dev_dyn_pack(rfx_ctx *ctx, const rfx_dyn_records *host_in, rfx_dyn_packed *d_out) try {
    if (!ctx || !host_in || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(dyn_pack_host(ctx, host_in, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_unpack(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_records *host_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !host_out) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    uint32_t lmin = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(dyn_check_lengths(ctx, a, &lmin));
    return dyn_unpack_host(ctx, a, host_out);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, int form, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text, d_row_off, n_rows) || (form != 0 && form != 1)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(dyn_binarize(ctx, d_text, d_row_off, n_rows, form, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_sort(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, rfx_dyn_packed *d_out, int64_t *d_part_start) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out) || !d_part_start || !parts_ok(P)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ps;
    uint32_t lmin = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(dyn_sort(ctx, a, P, b, ps, &lmin));
    RFX_TRY(dyn_store(ctx, b, d_out));
    return part_starts_store(ctx, d_part_start, ps, P);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_random_reflection(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const int64_t *d_part_start, int P, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out) || !d_part_start || !parts_ok(P)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    uint32_t lmin = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(dyn_check_lengths(ctx, a, &lmin));
    RFX_TRY(dyn_reflect(ctx, a, d_part_start, P, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_extend_pass(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const int64_t *d_part_start, int P, int stage, int start_iteration,
                            int start_marker, rfx_dyn_packed *d_out, int64_t *d_out_part_start) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out) || !d_part_start || !parts_ok(P) || (stage != 0 && stage != 1) ||
        (start_marker != 1 && start_marker != 2))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ops;
    uint32_t lmin = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(dyn_check_lengths(ctx, a, &lmin));
    RFX_TRY(part_starts_alloc(ctx, ops, P, false));
    RFX_TRY(dyn_pass(ctx, a, d_part_start, P, lmin, stage, start_iteration, start_marker, b, ops.as<int64_t>()));
    RFX_TRY(dyn_store(ctx, b, d_out));
    return d_out_part_start ? part_starts_store(ctx, d_out_part_start, ops, P) : sync_checked(ctx);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_run(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, int random_reflection, int passes_first_four, int start_iteration,
                    int end_iteration, rfx_dyn_packed *d_out, int64_t *trace, int64_t trace_cap, int64_t *n_trace) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out) || !parts_ok(P) || passes_first_four < 0) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    uint32_t lmin = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(dyn_check_lengths(ctx, a, &lmin));
    RFX_TRY(dyn_run(ctx, a, P, random_reflection, passes_first_four, start_iteration, end_iteration, trace, trace_cap, n_trace));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_to_text(rfx_ctx *ctx, const rfx_dyn_packed *d_in, char *d_text, int64_t cap, int64_t *out_len) try {
    if (!ctx || !dyn_packed_ok(d_in) || !out_len || cap < 0 || (cap > 0 && !d_text)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    uint32_t lmin = 0;
    int64_t total = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(dyn_check_lengths(ctx, a, &lmin));
    RFX_TRY(dyn_to_text(ctx, a, d_text, cap, &total, nullptr));
    *out_len = total;
    return total > cap ? RFX_E_CAP : RFX_OK;
} RFX_API_CATCH(ctx)

// host text in, host text out; everything between packed and in HBM: upload, binarize, run, to-text, one copy back
int rfx_dyn_run_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int form, int P, int random_reflection,
                     int passes_first_four, int start_iteration, int end_iteration, char *out, int64_t cap, int64_t *out_len, int64_t *trace,
                     int64_t trace_cap, int64_t *n_trace) try {
    if (!ctx || !text_rows_ok(text, row_off, n_rows) || (form != 0 && form != 1) || !parts_ok(P) || passes_first_four < 0 ||
        !out_len || cap < 0 || (cap > 0 && !out))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_text, d_off, d_out;
    DynDev a;
    int64_t total = 0;
    RFX_TRY(dyn_upload_text(ctx, text, row_off, n_rows, d_text, d_off));
    RFX_TRY(dyn_binarize(ctx, (const char *)d_text.p, d_off.as<int64_t>(), n_rows, form, a));
    RFX_TRY(dyn_run(ctx, a, P, random_reflection, passes_first_four, start_iteration, end_iteration, trace, trace_cap, n_trace));
    RFX_TRY(dyn_to_text(ctx, a, nullptr, 0, &total, &d_out));
    return text_to_host(ctx, {{d_out, total, out, cap, out_len}}, true);
} RFX_API_CATCH(ctx)

// ---- the host forms: pack -> the same kernels -> unpack -----------------------------------------------------------------------
int rfx_dyn_binarize(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int form, rfx_dyn_records *out) try {
    if (!ctx || !out || !text_rows_ok(text, row_off, n_rows) || (form != 0 && form != 1)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_text, d_off;
    DynDev a;
    RFX_TRY(dyn_upload_text(ctx, text, row_off, n_rows, d_text, d_off));
    RFX_TRY(dyn_binarize(ctx, (const char *)d_text.p, d_off.as<int64_t>(), n_rows, form, a));
    return dyn_unpack_host(ctx, a, out);
} RFX_API_CATCH(ctx)

int rfx_dyn_sort(rfx_ctx *ctx, const rfx_dyn_records *in, int P, rfx_dyn_records *out, int64_t *part_start) try {
    if (!ctx || !in || !out || !part_start || !parts_ok(P)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ps;
    uint32_t lmin = 0;
    RFX_TRY(dyn_pack_host(ctx, in, a));
    RFX_TRY(dyn_sort(ctx, a, P, b, ps, &lmin));
    RFX_TRY(dyn_unpack_host(ctx, b, out));
    RFX_HIP(hipMemcpyAsync(part_start, ps.p, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

int rfx_dyn_random_reflection(rfx_ctx *ctx, const rfx_dyn_records *in, const int64_t *part_start, int P, rfx_dyn_records *out) try {
    if (!ctx || !in || !out || !part_start || !parts_ok(P)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ps;
    RFX_TRY(dyn_pack_host(ctx, in, a));
    RFX_ALLOC(ps, int64_t, P + 1);
    RFX_HIP(hipMemcpyAsync(ps.p, part_start, (size_t)(P + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    RFX_TRY(dyn_reflect(ctx, a, ps.as<int64_t>(), P, b));
    return dyn_unpack_host(ctx, b, out);
} RFX_API_CATCH(ctx)

int rfx_dyn_extend_pass(rfx_ctx *ctx, const rfx_dyn_records *in, const int64_t *part_start, int P, int stage, int start_iteration,
                        int start_marker, rfx_dyn_records *out, int64_t *out_part_start) try {
    if (!ctx || !in || !out || !part_start || !parts_ok(P) || (stage != 0 && stage != 1) || (start_marker != 1 && start_marker != 2))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ps, ops;
    RFX_TRY(dyn_pack_host(ctx, in, a));
    RFX_ALLOC(ps, int64_t, P + 1); RFX_ALLOC(ops, int64_t, P + 1);
    RFX_HIP(hipMemcpyAsync(ps.p, part_start, (size_t)(P + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    int64_t lmin = INT64_MAX;
    for (int64_t i = 0; i < in->n; i++) lmin = std::min(lmin, in->key_off[i + 1] - in->key_off[i]);
    if (in->n == 0) lmin = 0;
    RFX_TRY(dyn_pass(ctx, a, ps.as<int64_t>(), P, (uint32_t)lmin, stage, start_iteration, start_marker, b, ops.as<int64_t>()));
    RFX_TRY(dyn_unpack_host(ctx, b, out));
    if (out_part_start) RFX_HIP(hipMemcpyAsync(out_part_start, ops.p, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

int rfx_dyn_run(rfx_ctx *ctx, const rfx_dyn_records *in, int P, int random_reflection, int passes_first_four, int start_iteration,
                int end_iteration, rfx_dyn_records *out, int64_t *trace, int64_t trace_cap, int64_t *n_trace) try {
    if (!ctx || !in || !out || !parts_ok(P) || passes_first_four < 0) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(dyn_pack_host(ctx, in, a));
    RFX_TRY(dyn_run(ctx, a, P, random_reflection, passes_first_four, start_iteration, end_iteration, trace, trace_cap, n_trace));
    return dyn_unpack_host(ctx, a, out);
} RFX_API_CATCH(ctx)

// ---- the Row form of the third layout (what a JNI shim converts between) -----------------------------------------------

// left-aligned 31-base blocks with a 01 terminator -> base codes; returns the length (currentKmerSizeFromBinaryBlockArray,
// FirstFour:2301-2311), or -1 when cap is short
int rfx_dyn_blocks_to_bases(const int64_t *blocks, int n_blocks, uint8_t *out, int cap) try {
    if (!blocks || n_blocks < 1) return -1;
    const uint64_t last = (uint64_t)blocks[n_blocks - 1];
    const int tz = last ? __builtin_ctzll(last) : 64;
    const int len = (n_blocks - 1) * 31 + (32 - tz / 2 - 1);
    if (len > cap) return -1;
    for (int i = 0; i < len; i++) out[i] = (uint8_t)(((uint64_t)blocks[i / 31] >> (2 * (31 - i % 31))) & 3);
    return len < 0 ? 0 : len;
} RFX_API_CATCH(nullptr)
// base codes -> blocks; returns the number of blocks ((n - 1) / 31 + 1), or -1 when cap is short
int rfx_dyn_bases_to_blocks(const uint8_t *bases, int n, int64_t *out, int cap) try {
    const int nb = n <= 0 ? 1 : (n - 1) / 31 + 1;
    if (nb > cap || !out) return -1;
    for (int j = 0; j < nb; j++) {
        uint64_t x = 0;
        const int b0 = 31 * j;
        int m = n - b0;
        if (m > 31) m = 31;
        if (m < 0) m = 0;
        for (int i = 0; i < m; i++) x |= (uint64_t)bases[b0 + i] << (2 * (31 - i));
        if (b0 + 31 >= n) x |= 1ULL << (2 * (31 - m));
        out[j] = (int64_t)x;
    }
    return nb;
} RFX_API_CATCH(nullptr)
// buildingAlongFromThreeInt (FirstFour:2340-2366) and getReflexivMarker / getLeftMarker / getRightMarker (:2313-2338)
int64_t rfx_dyn_attribute(int marker, int left, int right) try {
    if (left >= 30000) left = 30000; else if (left <= -30000) left = 60000; else if (left < 0) left = 30000 - left;
    if (right >= 30000) right = 30000; else if (right <= -30000) right = 60000; else if (right < 0) right = 30000 - right;
    return (int64_t)(((uint64_t)(uint32_t)marker << 62) | ((uint64_t)(uint32_t)left << 32) | (uint64_t)(uint32_t)right);
} RFX_API_CATCH(nullptr)
void rfx_dyn_attribute_unpack(int64_t a, int *marker, int *left, int *right) try {
    if (marker) *marker = (int)((uint64_t)a >> 62);
    int l = (int)((uint64_t)a >> 32) & ~(3 << 30);
    if (l > 30000) l = 30000 - l;
    int r = (int)a;
    if (r > 30000) r = 30000 - r;
    if (left) *left = l;
    if (right) *right = r;
} RFX_API_CATCH_VOID(nullptr)

}  // extern "C"
