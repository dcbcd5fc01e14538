// rfx_endmap.hip -- reads onto the contig ends (the front half of the Mapping stage) on packed sets that stay in HBM (DESIGN.md section
// 26).  The reference pipes every read through an external aligner and a script it does not ship (P/ReflexivDSDynamicKmerMapping.java
// :162-223, :1157-1266); this stage has semantics of its OWN, written down in section 26 and in include/reflexiv_hip.h: an ungapped
// end-overhang mapper that emits exactly the rows rfx_dev_endext_consensus uses.  Nothing here is the reference's:
//   index        the layout check in a launch of its own; then one thread per target end: the end's seed and its reverse complement as
//                2 * seed bit values with the tag 2 * end + orientation, a bit of each hashed filter; a key sort makes the table (equal
//                keys in tag order)
//   scan         ONE pass over the packed reads, a thread per read, run twice (count, then fill behind a scan of the counts): the
//                rolling seed value in a register, shifted and masked per base; the filter in LDS rejects a window without leaving
//                the CU, a second filter of 2 MB (one load, L2) most of what it lets through; a window that passes both is looked up
//                in the table (a binary search, L2) and every placement of it is verified 32 bases a step (pk_mismatch32); the fill
//                orders a read's rows by strand, end and offset
//   text         as k_fx2_text_fill: sizes, a scan, one read-back, one thread per 16-byte chunk cut at the destination ADDRESS; the
//                reverse complement of a read comes out of its words (pk_rc_seg32)
#include <algorithm>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

namespace {

#define MP_END 200                   // bases of a contig end; a contig of 2 MP_END bases or more gives two targets (rfx_fixing2.hip FX2_END)
#define MP_FILTER_BITS 18            // the hashed bit filter: 2^18 bits = 32 KB of LDS a workgroup
#define MP_FILTER_WORDS (1 << (MP_FILTER_BITS - 5))
#define MP_FILTER2_BITS 24           // the second filter behind it, another hash: 2^24 bits = 2 MB in HBM, which L2 holds
#define MP_FILTER2_WORDS (1 << (MP_FILTER2_BITS - 5))
#define MP_BLOCK 256

// what is wrong with a call's input (CallFlags::bad)
enum { MP_BAD_LAYOUT = 1, MP_TOO_LONG = 2, MP_BAD_READ = 4, MP_BAD_HIT = 8 };

__device__ __forceinline__ uint32_t mp_hash(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - MP_FILTER_BITS)); }
__device__ __forceinline__ uint32_t mp_hash2(uint64_t key) { return (uint32_t)((key * 0xC2B2AE3D27D4EB4Full) >> (64 - MP_FILTER2_BITS)); }
// the target of a contig of L bases: its length, and whether it is the whole contig (both ends on one target)
__device__ __forceinline__ int mp_target_len(int L) { return L < 2 * MP_END ? L : MP_END; }

// ---- index ---------------------------------------------------------------------------------------------------------------------------
// one thread per contig: the layout the header promises, checked in a launch of its own BEFORE anything indexes with it -- word_off[0]
// = 0 and every contig on exactly ceil(len / 32) words make every offset the sum of those in front of it
__global__ __launch_bounds__(256) void k_mp_check(const Fx2View c, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    const int64_t L = c.len[i];
    const bool bad = L < 0 || c.woff[i + 1] - c.woff[i] != ((L + 31) >> 5) || (i == 0 && c.woff[0] != 0);
    if (bad) atomicOr(&flags->bad, (uint32_t)MP_BAD_LAYOUT);
    else if (L >= ((int64_t)1 << 30)) atomicOr(&flags->bad, (uint32_t)MP_TOO_LONG);
}
// one thread per end e = 2 contig + side: table entries 2 e (the seed, strand 0) and 2 e + 1 (its reverse complement, strand 1); an end
// that does not exist (a contig below `seed` bases) gets the key 2^(2 seed), which no window has
__global__ __launch_bounds__(256) void k_mp_seeds(const Fx2View c, int seed, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                  uint32_t *__restrict__ filter, uint32_t *__restrict__ filter2) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * c.n) return;
    const int64_t i = e >> 1;
    const int L = (int)c.len[i], side = (int)(e & 1);
    const uint64_t none = 1ull << (2 * seed);
    uint64_t fw = none, rc = none;
    if (L >= seed) {
        const uint64_t front = pk_keep(pk_seg32(c.w + c.woff[i], L, side ? L - seed : 0), seed);      // the seed at the front of a word
        fw = front >> (64 - 2 * seed);
        rc = ~pk_rev2(front) & (none - 1);                          // turned round it sits at the back; the complement of its bits only
        const uint32_t h0 = mp_hash(fw), h1 = mp_hash(rc), g0 = mp_hash2(fw), g1 = mp_hash2(rc);
        atomicOr(&filter[h0 >> 5], 1u << (h0 & 31));
        atomicOr(&filter[h1 >> 5], 1u << (h1 & 31));
        atomicOr(&filter2[g0 >> 5], 1u << (g0 & 31));
        atomicOr(&filter2[g1 >> 5], 1u << (g1 & 31));
    }
    keys[2 * e] = fw; vals[2 * e] = (uint32_t)(2 * e);
    keys[2 * e + 1] = rc; vals[2 * e + 1] = (uint32_t)(2 * e + 1);
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------------
struct MpReads { const uint64_t *w; const uint32_t *len; int64_t n; int wpr; };
struct MpTable { const uint64_t *keys; const uint32_t *vals; int64_t m; };

// the placement of a read of n bases whose forward window at base j has the table entry `tag`: valid -> 1 (written at `at` when FILL)
template <bool FILL>
__device__ __forceinline__ uint32_t mp_try(const Fx2View &c, const rfx_map_params &p, const uint64_t *__restrict__ rw, int n, int64_t read, int j,
                                           uint32_t tag, const MpHits &o, int64_t at) {
    const int end = (int)(tag >> 1), strand = (int)(tag & 1u), side = end & 1;
    const int64_t ci = end >> 1;
    const int L = (int)c.len[ci], tlen = mp_target_len(L);
    const int off = strand ? n - p.seed - j : j;                    // where the seed sits in the orientation that matched
    int v, rs, cs, past;                                            // overlap, its start in the read and in the contig, read bases past the FAR end
    if (side == 0) {
        if (off < 1) return 0u;                                     // (off <= n - seed by the window)
        v = min(n - off, tlen); past = n - off - v; rs = off; cs = 0;
    } else {
        if (off > n - 1 - p.seed) return 0u;                        // (off >= 0 by the window)
        v = min(off + p.seed, tlen); past = off + p.seed - v; rs = past; cs = L - v;
    }
    if (v < p.min_overlap || (L < 2 * MP_END && past > 0)) return 0u;       // too short / a whole-contig target with bases past both ends
    const uint64_t *cw = c.w + c.woff[ci];
    int mm = 0;
    for (int t = 0; t < v && mm <= p.max_mismatch; t += 32) {
        const uint64_t a = strand ? pk_rc_seg32(rw, n, rs + t) : pk_seg32(rw, n, rs + t);
        mm += pk_mismatch32(a, pk_seg32(cw, L, cs + t), v - t);
    }
    if (mm > p.max_mismatch) return 0u;
    if (FILL) { o.read[at] = (int32_t)read; o.end[at] = end; o.strand[at] = strand; o.off[at] = off; o.v[at] = v; }
    return 1u;
}
// the order of a read's rows: strand, end, offset
__device__ __forceinline__ uint64_t mp_order(const MpHits &o, int64_t q) {
    return ((uint64_t)o.strand[q] << 62) | ((uint64_t)(uint32_t)o.end[q] << 31) | (uint64_t)(uint32_t)o.off[q];
}

// a thread per read, a workgroup per MP_BLOCK reads at a time.  !FILL: cnt[i] = the valid placements of read i.  FILL: they are written
// from hoff[i] on, then put in order (an insertion sort by the thread that found them: a read has a handful)
template <bool FILL>
__global__ __launch_bounds__(MP_BLOCK) void k_mp_scan(const Fx2View c, const MpReads rd, const rfx_map_params p, const MpTable tb,
                                                      const uint32_t *__restrict__ gfilter, const uint32_t *__restrict__ filter2,
                                                      uint32_t *__restrict__ cnt,
                                                      const uint64_t *__restrict__ hoff, const MpHits o, CallFlags *__restrict__ flags) {
    __shared__ __attribute__((aligned(16))) uint32_t filter[MP_FILTER_WORDS];
    for (int t = (int)threadIdx.x; t < MP_FILTER_WORDS / 4; t += MP_BLOCK)
        reinterpret_cast<uint4 *>(filter)[t] = reinterpret_cast<const uint4 *>(gfilter)[t];
    __syncthreads();
    const uint64_t mask = (1ull << (2 * p.seed)) - 1;
    for (int64_t i = (int64_t)blockIdx.x * MP_BLOCK + threadIdx.x; i < rd.n; i += (int64_t)gridDim.x * MP_BLOCK) {
        const uint32_t n32 = rd.len[i];
        if (n32 > 32u * (uint32_t)rd.wpr) {                         // the words do not hold it: the call fails
            if (!FILL) { atomicOr(&flags->bad, (uint32_t)MP_BAD_READ); cnt[i] = 0u; }
            continue;
        }
        const int n = (int)n32;
        const uint64_t *rw = rd.w + i * rd.wpr;
        const int64_t at = FILL ? (int64_t)hoff[i] : 0;
        uint32_t found = 0u;
        uint64_t roll = 0ull;
        for (int k = 0; 32 * k < n; k++) {
            uint64_t x = rw[k];
            const int m = min(32, n - 32 * k);
            for (int b = 0; b < m; b++) {
                roll = ((roll << 2) | (x >> 62)) & mask;
                x <<= 2;
                const int j = 32 * k + b - p.seed + 1;              // the window ends at this base
                if (j < 0) continue;
                const uint32_t h = mp_hash(roll);
                if (!((filter[h >> 5] >> (h & 31)) & 1u)) continue;
                const uint32_t g = mp_hash2(roll);
                if (!((filter2[g >> 5] >> (g & 31)) & 1u)) continue;
                int64_t lo = 0, hi = tb.m;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (tb.keys[mid] < roll) lo = mid + 1; else hi = mid;
                }
                for (; lo < tb.m && tb.keys[lo] == roll; lo++) found += mp_try<FILL>(c, p, rw, n, i, j, tb.vals[lo], o, at + found);
            }
        }
        if (!FILL) { cnt[i] = found; continue; }
        for (int64_t q = at + 1; q < at + found; q++) {
            const uint64_t key = mp_order(o, q);
            const int32_t e = o.end[q], s = o.strand[q], f = o.off[q], v = o.v[q];
            int64_t r = q;
            while (r > at && mp_order(o, r - 1) > key) {
                o.end[r] = o.end[r - 1]; o.strand[r] = o.strand[r - 1]; o.off[r] = o.off[r - 1]; o.v[r] = o.v[r - 1];
                r--;
            }
            o.end[r] = e; o.strand[r] = s; o.off[r] = f; o.v[r] = v;
        }
    }
}

// ---- text: the rows "name \t start \t cigar \t seq \n" -------------------------------------------------------------------------------
// name = Contig_<L>_<left>_<right>_<idx>, -L or -R behind it for an end of MP_END bases; the CIGAR's three parts (a part of 0 is left
// out: only the clip at the far end can be); seq = the read in the orientation that matched
struct MpHitsIn { int64_t n; const int32_t *read, *end, *strand, *off, *v; int seed; };
struct MpRow { int f0, f1, f2, f3, suf, start, c0, c1, c2, n, strand, bytes; const uint64_t *rw; };
__device__ __forceinline__ int mp_field(const MpRow &r, int k) { return k == 0 ? r.f0 : k == 1 ? r.f1 : k == 2 ? r.f2 : r.f3; }
__device__ __forceinline__ int mp_part(const MpRow &r, int k) { return k == 0 ? r.c0 : k == 1 ? r.c1 : r.c2; }
// ok: the hit is one that rfx_dev_map_ends can have written for these contigs and this read (everything the row indexes with)
__device__ __forceinline__ MpRow mp_row(const Fx2View &c, const MpReads &rd, const MpHitsIn &h, int64_t q, bool *ok) {
    MpRow r{};
    const int end = h.end[q], strand = h.strand[q], off = h.off[q], v = h.v[q];
    const int64_t read = h.read[q];
    *ok = false;
    if (end < 0 || (int64_t)end >= 2 * c.n || (strand & ~1) || read < 0) return r;
    const int64_t ci = end >> 1, L64 = c.len[ci];
    if (L64 < h.seed || L64 >= ((int64_t)1 << 30) || c.woff[ci + 1] - c.woff[ci] != ((L64 + 31) >> 5)) return r;
    const uint32_t n32 = rd.len[read];
    if (n32 > 32u * (uint32_t)rd.wpr) return r;
    const int L = (int)L64, n = (int)n32, tlen = mp_target_len(L), side = end & 1;
    int past, over;                                                 // the clips at the far end and at this end
    if (side == 0) {
        if (off < 1 || off > n - h.seed || v != min(n - off, tlen)) return r;
        over = off; past = n - off - v;
    } else {
        if (off < 0 || off > n - 1 - h.seed || v != min(off + h.seed, tlen)) return r;
        over = n - off - h.seed; past = off + h.seed - v;
    }
    *ok = true;
    r.f0 = L; r.f1 = c.left[ci]; r.f2 = c.right[ci]; r.f3 = (int)ci;
    r.suf = L < 2 * MP_END ? 0 : 1 + side;
    r.start = side ? tlen - v + 1 : 1;
    r.c0 = side ? past : over; r.c1 = v; r.c2 = side ? over : past;
    r.n = n; r.strand = strand; r.rw = rd.w + read * rd.wpr;
    int b = 7 + (r.suf ? 2 : 0) + 3 + 3 + pk_int_chars(r.start) + n + 1;      // "Contig_", the suffix, three '_', three tabs, the newline
#pragma unroll
    for (int k = 0; k < 4; k++) b += pk_int_chars(mp_field(r, k));
#pragma unroll
    for (int k = 0; k < 3; k++) b += mp_part(r, k) ? pk_int_chars(mp_part(r, k)) + 1 : 0;
    r.bytes = b;
    return r;
}
// byte q of a row: a character, or (0) base *t of seq
__device__ __forceinline__ char mp_byte(const MpRow &r, int q, int *t) {
    if (q < 7) return "Contig_"[q];
    q -= 7;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int v = mp_field(r, k), ch = pk_int_chars(v);
        if (q < ch) return pk_int_char(v, q);
        q -= ch;
        if (k < 3) { if (q == 0) return '_'; q--; }
    }
    if (r.suf) { if (q < 2) return q == 0 ? '-' : r.suf == 1 ? 'L' : 'R'; q -= 2; }
    if (q == 0) return '\t';
    q--;
    const int sc = pk_int_chars(r.start);
    if (q < sc) return pk_int_char(r.start, q);
    q -= sc;
    if (q == 0) return '\t';
    q--;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int v = mp_part(r, k);
        if (!v) continue;
        const int ch = pk_int_chars(v);
        if (q < ch) return pk_int_char(v, q);
        q -= ch;
        if (q == 0) return k == 1 ? 'M' : 'S';
        q--;
    }
    if (q == 0) return '\t';
    q--;
    if (q < r.n) { *t = q; return 0; }
    return '\n';
}
// base t of seq / the 16 letters from base t (t + 16 <= n): out of the words in either orientation
__device__ __forceinline__ uint32_t mp_base(const MpRow &r, int t) { return r.strand ? 3u - pk_base_of(r.rw, r.n - 1 - t) : pk_base_of(r.rw, t); }
__device__ __forceinline__ Pk16 mp_letters16(const MpRow &r, int t) {
    if (!r.strand) return pk_letters16(r.rw, t);
    const uint64_t x[1] = {pk_rc_seg32(r.rw, r.n, t)};
    return pk_letters16(x, 0);
}
__global__ __launch_bounds__(256) void k_mp_text_sizes(const Fx2View c, const MpReads rd, const MpHitsIn h, uint64_t *__restrict__ sz,
                                                       CallFlags *__restrict__ flags) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= h.n) return;
    bool ok;
    const MpRow r = mp_row(c, rd, h, q, &ok);
    if (!ok) atomicOr(&flags->bad, (uint32_t)MP_BAD_HIT);
    sz[q] = ok ? (uint64_t)r.bytes : 0ull;
}
__global__ __launch_bounds__(256) void k_mp_row_off(const uint64_t *__restrict__ toff, int64_t n, int64_t *__restrict__ row_off) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n) row_off[q] = (int64_t)toff[q];
}
// one thread per 16-byte chunk of the destination (k_ee_text_fill): chunk ch holds the text's bytes [16 ch - skew, 16 ch - skew + 16)
// cut to [0, lim), skew = the destination address mod 16, so a whole chunk is a 16-byte-aligned store
__global__ __launch_bounds__(256) void k_mp_text_fill(const Fx2View c, const MpReads rd, const MpHitsIn h, const uint64_t *__restrict__ toff,
                                                      int64_t lim, int skew, int64_t chunks, char *__restrict__ out) {
    const int64_t ch = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= chunks) return;
    const int64_t start = 16 * ch - skew;
    const int64_t b0 = start < 0 ? 0 : start, b1 = start + 16 < lim ? start + 16 : lim;
    const bool whole = b1 - b0 == 16;
    int64_t i = pk_find(toff, h.n, b0);
    bool ok;
    MpRow r = mp_row(c, rd, h, i, &ok);
    int q = (int)(b0 - (int64_t)toff[i]);
    int64_t next = (int64_t)toff[i + 1];
    uint32_t o0 = 0u, o1 = 0u, o2 = 0u, o3 = 0u;
    int t = 0;
    const char first = mp_byte(r, q, &t);
    if (whole && first == 0 && t + 16 <= r.n) {
        const Pk16 y = mp_letters16(r, t);
        o0 = y.a; o1 = y.b; o2 = y.c; o3 = y.d;
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t b = b0 + j;
            if (b < b1) {
                if (b >= next) {                                  // the chunk crosses into the next row (every row has bytes)
                    i++;
                    r = mp_row(c, rd, h, i, &ok);
                    q = 0; next = (int64_t)toff[i + 1];
                }
                char cc = mp_byte(r, q, &t);
                if (cc == 0) cc = (char)pk_letter(mp_base(r, t));
                const uint32_t x = (uint32_t)(uint8_t)cc << (8 * (j & 3));
                if (j < 4) o0 |= x; else if (j < 8) o1 |= x; else if (j < 12) o2 |= x; else o3 |= x;
                q++;
            }
        }
    }
    if (whole) {
        *reinterpret_cast<uint4 *>(out + b0) = make_uint4(o0, o1, o2, o3);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t x = j < 4 ? o0 : j < 8 ? o1 : j < 12 ? o2 : o3;
            if (b0 + j < b1) out[b0 + j] = (char)(x >> (8 * (j & 3)));
        }
    }
}

int mp_bad(rfx_ctx *ctx, uint32_t bad) {
    if (bad & MP_BAD_LAYOUT) { ctx->last_error = "end mapping: a contig set whose word_off and len disagree"; return RFX_E_ARG; }
    if (bad & MP_TOO_LONG) { ctx->last_error = "end mapping: a contig of 2^30 bases or more"; return RFX_E_LIMIT; }
    if (bad & MP_BAD_READ) { ctx->last_error = "end mapping: a read longer than 32 * words_per_read bases"; return RFX_E_ARG; }
    if (bad & MP_BAD_HIT) { ctx->last_error = "end mapping: a hit that rfx_dev_map_ends does not write for these contigs and reads"; return RFX_E_ARG; }
    return RFX_OK;
}
unsigned mp_grid(rfx_ctx *ctx, int64_t n_reads) {
    return (unsigned)std::min<int64_t>(ceil_div(std::max<int64_t>(n_reads, 1), MP_BLOCK), 5 * (int64_t)std::max(ctx->num_cu, 1));      // (32 KB of LDS each: five on a CU)
}

}  // namespace

bool rfx::mp_params_ok(rfx_ctx *ctx, const rfx_map_params *p) {
    if (!p) return false;
    if (p->seed < 11 || p->seed > 31) { ctx->last_error = "end mapping: seed must be 11..31"; return false; }
    if (p->min_overlap < p->seed || p->min_overlap > MP_END) { ctx->last_error = "end mapping: min_overlap must be seed..200"; return false; }
    if (p->max_mismatch < 0 || p->max_mismatch > 31) { ctx->last_error = "end mapping: max_mismatch must be 0..31"; return false; }
    return true;
}

// the index, the counting pass and the scan of its counts: plan.hits = the rows of the call
int rfx::mp_plan(rfx_ctx *ctx, const Fx2View &c, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, const rfx_map_params &p,
                 MpPlan &plan) {
    plan.hits = 0; plan.m = 0;
    if (c.n >= ((int64_t)1 << 29)) { ctx->last_error = "end mapping: 2^29 contigs or more"; return RFX_E_LIMIT; }
    if (n_reads >= ((int64_t)1 << 31)) { ctx->last_error = "end mapping: 2^31 reads or more"; return RFX_E_LIMIT; }
    if (c.n == 0) return RFX_OK;
    const int64_t m = 4 * c.n;
    DevBuf tk, tv, flags;
    RFX_ALLOC(plan.keys, uint64_t, m); RFX_ALLOC(plan.vals, uint32_t, m); RFX_ALLOC(tk, uint64_t, m); RFX_ALLOC(tv, uint32_t, m);
    RFX_ALLOC(plan.filter, uint32_t, MP_FILTER_WORDS + MP_FILTER2_WORDS);       // (both filters: the second behind the first)
    RFX_ALLOC(plan.cnt, uint32_t, std::max<int64_t>(n_reads, 1)); RFX_ALLOC(plan.hoff, uint64_t, n_reads + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_mp_check, c.n, c, flags.as<CallFlags>());
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));      // (a refused layout is not indexed with)
    RFX_TRY(mp_bad(ctx, f.bad));
    RFX_HIP(hipMemsetAsync(plan.filter.p, 0, (MP_FILTER_WORDS + MP_FILTER2_WORDS) * sizeof(uint32_t), ctx->stream));
    RFX_LAUNCH_N(k_mp_seeds, 2 * c.n, c, p.seed, plan.keys.as<uint64_t>(), plan.vals.as<uint32_t>(), plan.filter.as<uint32_t>(),
                 plan.filter.as<uint32_t>() + MP_FILTER_WORDS);
    RFX_TRY(sort_pairs(ctx, plan.keys.as<uint64_t>(), plan.vals.as<uint32_t>(), m, 2 * p.seed + 1, tk.as<uint64_t>(), tv.as<uint32_t>()));
    plan.m = m;
    if (n_reads == 0) return RFX_OK;
    const MpReads rd{d_words, d_read_len, n_reads, wpr};
    const MpTable tb{plan.keys.as<uint64_t>(), plan.vals.as<uint32_t>(), m};
    RFX_LAUNCH(k_mp_scan<false>, dim3(mp_grid(ctx, n_reads)), dim3(MP_BLOCK), 0, c, rd, p, tb, plan.filter.as<uint32_t>(), plan.filter.as<uint32_t>() + MP_FILTER_WORDS,
               plan.cnt.as<uint32_t>(), nullptr, MpHits{}, flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, plan.cnt.as<uint32_t>(), plan.hoff.as<uint64_t>(), n_reads));
    RFX_TRY(call_flags_read(ctx, flags, plan.hoff.as<uint64_t>() + n_reads, nullptr, nullptr, &f));
    RFX_TRY(mp_bad(ctx, f.bad));
    if (f.total[0] >= ((uint64_t)1 << 31)) { ctx->last_error = "end mapping: 2^31 hits or more"; return RFX_E_LIMIT; }
    plan.hits = (int64_t)f.total[0];
    return RFX_OK;
}
// the rows into arrays that hold plan.hits entries each
int rfx::mp_fill(rfx_ctx *ctx, const Fx2View &c, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, const rfx_map_params &p,
                 const MpPlan &plan, const MpHits &o) {
    if (plan.hits == 0) return RFX_OK;
    const MpReads rd{d_words, d_read_len, n_reads, wpr};
    const MpTable tb{plan.keys.as<uint64_t>(), plan.vals.as<uint32_t>(), plan.m};
    RFX_LAUNCH(k_mp_scan<true>, dim3(mp_grid(ctx, n_reads)), dim3(MP_BLOCK), 0, c, rd, p, tb, plan.filter.as<uint32_t>(), plan.filter.as<uint32_t>() + MP_FILTER_WORDS,
               nullptr, plan.hoff.as<uint64_t>(), o, nullptr);
    return RFX_OK;
}

// the rows as text into d_text (filled up to cap, nothing at or past it) and their n + 1 offsets into d_row_off (nullptr: none); *total =
// the text's length; own: a buffer of the library's
int rfx::mp_text(rfx_ctx *ctx, const Fx2View &c, const uint64_t *d_words, const uint32_t *d_read_len, int wpr, const MpHits &hits, int64_t n, int seed,
                 char *d_text, int64_t cap, int64_t *total, int64_t *d_row_off, DevBuf *own) {
    *total = 0;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "end mapping: 2^31 hits or more"; return RFX_E_LIMIT; }
    if (n == 0) {
        if (d_row_off) RFX_HIP(hipMemsetAsync(d_row_off, 0, 8, ctx->stream));
        if (own) RFX_HIP(own->alloc(1, ctx->stream));
        return sync_checked(ctx);
    }
    const MpReads rd{d_words, d_read_len, 0, wpr};
    const MpHitsIn h{n, hits.read, hits.end, hits.strand, hits.off, hits.v, seed};
    DevBuf sz, toff, flags;
    RFX_ALLOC(sz, uint64_t, n); RFX_ALLOC(toff, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_mp_text_sizes, n, c, rd, h, sz.as<uint64_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u64(ctx, sz.as<uint64_t>(), toff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, toff.as<uint64_t>() + n, nullptr, nullptr, &f));
    RFX_TRY(mp_bad(ctx, f.bad));
    *total = (int64_t)f.total[0];
    if (own) {
        RFX_HIP(own->alloc((size_t)std::max<int64_t>(*total, 1), ctx->stream));
        d_text = own->as<char>(); cap = *total;
    }
    if (d_row_off) RFX_LAUNCH_N(k_mp_row_off, n + 1, toff.as<uint64_t>(), n, d_row_off);
    const int64_t lim = std::min<int64_t>(*total, cap);
    if (lim > 0) {
        const int skew = (int)((uintptr_t)d_text & 15);
        const int64_t chunks = ceil_div(lim + skew, 16);
        RFX_LAUNCH_N(k_mp_text_fill, chunks, c, rd, h, toff.as<uint64_t>(), lim, skew, chunks, d_text);
    }
    return sync_checked(ctx);
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------
namespace {
bool mp_hits_ok(const rfx_map_hits *h) { return h && h->read && h->end && h->strand && h->offset && h->v && h->cap_n >= 0; }
}  // namespace

extern "C" {

void rfx_map_default_params(rfx_map_params *p) try {
    if (!p) return;
    p->seed = 21; p->min_overlap = 31; p->max_mismatch = 2;
} RFX_API_CATCH_VOID(nullptr)

int rfx_dev_map_ends(rfx_ctx *ctx, const rfx_contigs_packed *d_contigs, const int32_t *d_left, const int32_t *d_right, const uint64_t *d_words,
                     const uint32_t *d_read_len, int64_t n_reads, int words_per_read, const rfx_map_params *params, rfx_map_hits *d_out) try {
    if (!ctx || !fx2_contigs_in_ok(d_contigs, d_left, d_right) || n_reads < 0 || (n_reads > 0 && (!d_words || !d_read_len)) || words_per_read < 1 ||
        !mp_hits_ok(d_out) || !mp_params_ok(ctx, params))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    const Fx2View v = fx2_view(d_contigs, d_left, d_right);
    MpPlan plan;
    RFX_TRY(mp_plan(ctx, v, d_words, d_read_len, n_reads, words_per_read, *params, plan));
    if (!packed_out_fits(d_out, plan.hits)) return RFX_E_CAP;
    RFX_TRY(mp_fill(ctx, v, d_words, d_read_len, n_reads, words_per_read, *params, plan, mp_hits(d_out)));
    d_out->n = plan.hits; d_out->seed = params->seed;
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

int rfx_dev_map_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_contigs, const int32_t *d_left, const int32_t *d_right, const uint64_t *d_words,
                        const uint32_t *d_read_len, int words_per_read, const rfx_map_hits *hits, char *d_text, int64_t cap, int64_t *out_len,
                        int64_t *d_row_off, int64_t cap_rows) try {
    if (!ctx || !fx2_contigs_in_ok(d_contigs, d_left, d_right) || words_per_read < 1 || !mp_hits_ok(hits) || hits->n < 0 || hits->n > hits->cap_n ||
        (hits->n > 0 && (!d_words || !d_read_len || hits->seed < 11 || hits->seed > 31)) || !text_out_ok(d_text, cap, out_len) || !d_row_off || cap_rows < 0)
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    const bool rows_fit = cap_rows >= hits->n + 1;
    int64_t total = 0;
    // too few row offsets: the sizes only (a text buffer of 0 bytes takes nothing)
    RFX_TRY(mp_text(ctx, fx2_view(d_contigs, d_left, d_right), d_words, d_read_len, words_per_read, mp_hits(hits), hits->n, hits->seed, d_text,
                    rows_fit ? cap : 0, &total, rows_fit ? d_row_off : nullptr, nullptr));
    *out_len = total;
    return total > cap || !rows_fit ? RFX_E_CAP : RFX_OK;
} RFX_API_CATCH(ctx)

// host form: the text of 05FixingAgain and ASCII reads in, the row text out; everything between packed and in HBM: one upload each, the
// contigs and the read store, the index, both passes, the text, one copy back
int rfx_map_text(rfx_ctx *ctx, const char *contig_text, const int64_t *contig_off, int64_t n_contigs, const uint8_t *bases, const int64_t *read_off,
                 int64_t n_reads, const rfx_map_params *params, char *out, int64_t cap, int64_t *out_len) try {
    if (!ctx || !text_rows_ok(contig_text, contig_off, n_contigs) || !text_rows_ok((const char *)bases, read_off, n_reads) || !text_out_ok(out, cap, out_len) ||
        !mp_params_ok(ctx, params))
        return RFX_E_ARG;
    if (n_contigs >= ((int64_t)1 << 29) || n_reads >= ((int64_t)1 << 31)) {       // (before an offset is read or a byte uploaded)
        ctx->last_error = "end mapping: 2^29 contigs or 2^31 reads, or more";
        return RFX_E_LIMIT;
    }
    int64_t longest = 1;
    for (int64_t i = 0; i < n_reads; i++) longest = std::max(longest, read_off[i + 1] - read_off[i]);
    if (longest >= ((int64_t)1 << 30)) { ctx->last_error = "end mapping: a read of 2^30 bases or more"; return RFX_E_LIMIT; }
    RFX_HIP(hipSetDevice(ctx->device));
    const int wpr = (int)((longest + 31) >> 5);
    DevBuf d_ct, d_co, d_b, d_ro, d_words, d_len, d_rows;
    CtgDev ctg;
    MpHitsDev hits;
    RFX_TRY(dyn_upload_text(ctx, contig_text, contig_off, n_contigs, d_ct, d_co));
    RFX_TRY(dyn_upload_text(ctx, (const char *)bases, read_off, n_reads, d_b, d_ro));
    RFX_TRY(ee_contigs_from_rows(ctx, (const char *)d_ct.p, d_co.as<int64_t>(), n_contigs, ctg));
    const int64_t r1 = std::max<int64_t>(n_reads, 1);
    RFX_ALLOC(d_words, uint64_t, r1 * wpr); RFX_ALLOC(d_len, uint32_t, r1);
    if (n_reads > 0) RFX_TRY(encode_reads(ctx, d_b.as<uint8_t>(), d_ro.as<int64_t>(), n_reads, wpr, d_words.as<uint64_t>(), d_len.as<uint32_t>()));
    const Fx2View v = fx2_view(ctg);
    MpPlan plan;
    RFX_TRY(mp_plan(ctx, v, d_words.as<uint64_t>(), d_len.as<uint32_t>(), n_reads, wpr, *params, plan));
    RFX_TRY(mp_hits_alloc(ctx, hits, plan.hits));
    RFX_TRY(mp_fill(ctx, v, d_words.as<uint64_t>(), d_len.as<uint32_t>(), n_reads, wpr, *params, plan, mp_hits(hits)));
    int64_t total = 0;
    RFX_TRY(mp_text(ctx, v, d_words.as<uint64_t>(), d_len.as<uint32_t>(), wpr, mp_hits(hits), plan.hits, params->seed, nullptr, 0, &total, nullptr, &d_rows));
    return text_to_host(ctx, {{d_rows, total, out, cap, out_len}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"
