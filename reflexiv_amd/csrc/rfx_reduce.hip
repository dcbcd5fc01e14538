// rfx_reduce.hip -- the k-mer reduction stage (Count_<k1>_reduced and the rewritten Count_<k2>_sorted / _reduced) on packed record
// sets that stay in HBM: P/ReflexivDSDynamicKmerRuduction.java, driver `assemblyFromKmer` :143-287 --
// DynamicKmerBinarizerFromSorted (:3175-3303) on both inputs, union (the longer set first, :202),
// LeftLongerToShorterComparisonPreparation (:860-888), sort("k-1"), LeftLongerKmerVariantAdjustment (:1889-2245),
// RightLongerToShorterComparisonAndNeutralizationPreparation (:509-545), sort("k-1"),
// RightLongerKmerVariantAdjustmentAndNeutralization (:1203-1574), DSSubKmerToFullKmer (:2923-2968), sort("k"),
// ShorterKmerNeutralization (:2563-2731, the live code) and DSBinaryFullKmerArrayToStringShort / ...Long (:289-316, :401-428).
//
// The record sets are rfx_dyn_packed (rfx_dynamic.hip): four key words per record, 32 bases per word, the first base in the two
// highest bits, every bit past the last base 0 and every unused key word 0 -- every producer here writes those zeros.  A sub-k-mer
// set has ONE extension base at the top of ONE word per record (ext_off[i] = i), a full k-mer set has no extension words.  The
// three sorts are rfx_dynamic.hip's (dyn_sort, unchanged), the full k-mers and the text writer rfx_ksort.hip's (ks_set_full_kmers,
// ks_set_to_text: DSSubKmerToFullKmer and the two string classes are the sorting stage's, line for line).
//
// The two adjustments are three-row windows whose state -- the number of pending rows, 0, 1 or 2 -- does NOT reset at a new key,
// only at a partition's first row: rfx_reduce_fsm.h has the transition, shared with a host program.  k_rd_window (one thread per
// row: the three rows' lengths, prefix tests and extension equalities into nine bits, the row's map {0,1,2} -> {0,1,2} into six),
// then the scan of the maps under composition in three launches -- k_rd_scan_reduce (a block's composite), k_rd_scan_aggs (one block
// over the n / 256 composites), k_rd_scan_apply (the state ahead of every row, and how many records the row writes) -- with no
// kernel waiting on another workgroup, a scan of the counts, and k_rd_emit (a row writes its 0..3 records; the row that ends a
// partition also writes the flush).  The map of a partition's first row is constant, so the composition cuts itself there.
//
// The neutralizer keeps a row or not by comparing it with the last KEPT row.  With two lengths in play: a long row is always kept;
// a short row is dropped while every row since the nearest long row before it (in its partition) is a short prefix of that long
// row; a short row that was kept is taken out again when the next row of its partition is a long row it is a prefix of.  The
// nearest long row comes from a scan of the long flags and a scatter of the long rows' indices, the stretch's AND from a scan of
// the rows that break it, then a compaction.
//
// DEVIATION from the reference, stated in the header too: one call handles ONE pair.  A row whose k-mer is neither k1 nor k2 long
// is dropped at the binarizer; the reference would carry a row of another LISTED length through (its pipeline never writes one).
// A malformed attribute reads as rfx_dyn_binarize reads it (missing numbers are 0) where the reference throws.
#include <algorithm>
#include <string>
#include <vector>
#include "rfx_internal.h"
#include "rfx_packed_words.h"
#include "rfx_reduce_fsm.h"

using namespace rfx;

namespace {

#define RD_KW PK_KW

// what is wrong with a call's input (CallFlags::bad)
enum { RD_BAD_OFFSETS = 1, RD_BAD_COMMA = 2, RD_BAD_LEN = 4, RD_BAD_EXT = 8 };
// a row's word of the window pass: bit 0 the row opens a partition, bit 1 it ends one, bits 8..16 the nine bits of
// rfx_reduce_fsm.h for rows i - 2, i - 1, i, bits 20..21 the state ahead of the row
enum { RD_START = 1, RD_END = 2, RD_IN_SHIFT = 8, RD_STATE_SHIFT = 20 };

struct RdParams { int k1, k2; };

// (the word forms -- Pk4, pk_reverse, pk_prefix, pk_shl, pk_keep4 -- are rfx_packed_words.h's)
// the partition of row i: the largest p < P with ps[p] <= i (ps[0] = 0); its rows are [ps[p], ps[p + 1])
__device__ __forceinline__ int rd_part_of(const int64_t *__restrict__ ps, int P, int64_t i) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ps[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- step 1: DynamicKmerBinarizerFromSorted, and the union ----------------------------------------------------------------------------
// One thread per row "KMER,marker|left|right": the row ends ahead of its newline, the first ',' cuts it, a leading '(' of the k-mer
// and a trailing ')' of the attribute are dropped; keep = the k-mer has k1 or k2 letters; left / right clamped to +-30000.
__global__ __launch_bounds__(256) void k_rd_bin_sizes(const char *__restrict__ text, const int64_t *__restrict__ row_off, int64_t n, const RdParams prm,
                                                      uint32_t *__restrict__ keep, int64_t *__restrict__ kbeg, int32_t *__restrict__ mlr,
                                                      CallFlags *__restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int64_t b = row_off[r], e = row_off[r + 1];
    uint32_t bad = 0;
    if (e < b || b < 0) { bad |= RD_BAD_OFFSETS; e = b = 0; }
    while (e > b && (text[e - 1] == '\n' || text[e - 1] == '\r')) e--;
    int64_t c = b;
    while (c < e && text[c] != ',') c++;
    uint32_t kp = 0;
    if (c >= e) bad |= bad ? 0 : RD_BAD_COMMA;
    else {
        int64_t kb = b, ae = e;
        if (kb < c && text[kb] == '(') kb++;
        if (ae > c + 1 && text[ae - 1] == ')') ae--;
        int64_t i = c + 1;
        const int m = pk_parse_int(text, i, ae), l = pk_parse_int(text, i, ae), rr = pk_parse_int(text, i, ae);
        mlr[3 * r] = m;
        mlr[3 * r + 1] = pk_clamp(l);
        mlr[3 * r + 2] = pk_clamp(rr);
        kp = (c - kb == prm.k1 || c - kb == prm.k2) ? 1u : 0u;
        kbeg[r] = kb;
        keep[r] = (uint32_t)(kp ? c - kb : 0);                          // (the length of a kept row, 0 of a dropped one)
    }
    if (bad) { keep[r] = 0; atomicOr(&flags->bad, bad); }
}
__global__ __launch_bounds__(256) void k_rd_bin_flag(const uint32_t *__restrict__ len, int64_t n, uint32_t *__restrict__ keep) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) keep[r] = len[r] ? 1u : 0u;
}
// a kept row writes full k-mer record base + (its rank among the kept rows): the whole k-mer as the key, no extension
__global__ __launch_bounds__(256) void k_rd_bin_emit(const char *__restrict__ text, int64_t n, const uint32_t *__restrict__ len,
                                                     const uint64_t *__restrict__ slot, const int64_t *__restrict__ kbeg, const int32_t *__restrict__ mlr,
                                                     int64_t base, const DynOut o) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || !len[r]) return;
    const int k = (int)len[r];
    const char *s = text + kbeg[r];
    Pk4 f{0, 0, 0, 0};
    for (int j = 0; j < k; j++) {
        const char ch = s[j];
        pk_or(f, j >> 5, pk_at(pk_code(ch), j));
    }
    const int64_t q = base + (int64_t)slot[r];
    pk_store(o.key, q, f);
    o.key_len[q] = (uint8_t)k;
    o.ext_off[q] = 0;
    o.ext_len[q] = 0;
    o.marker[q] = mlr[3 * r]; o.left[q] = mlr[3 * r + 1]; o.right[q] = mlr[3 * r + 2];
}

// the same record from a packed set of full k-mers (rfx_dev_reduce_union_packed): one thread per input record, a kept one writes
// record base + (its rank among the kept) -- what k_ks_text_fill prints of it and k_rd_bin_sizes / k_rd_bin_emit read back: the key's
// bases (nothing behind them), the marker through its decimal text, left / right through theirs and clamped, no extension
__global__ __launch_bounds__(256) void k_rd_pk_emit(const DynView v, int64_t n, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank,
                                                    int64_t base, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int64_t q = base + (int64_t)rank[i];
    const int len = (int)v.key_len[i];
    pk_store(o.key, q, pk_keep4(pk_load(v.key, i), len));
    o.key_len[q] = (uint8_t)len;
    o.ext_off[q] = 0;
    o.ext_len[q] = 0;
    o.marker[q] = pk_int_as_text(v.marker[i]); o.left[q] = pk_clamp(pk_int_as_text(v.left[i])); o.right[q] = pk_clamp(pk_int_as_text(v.right[i]));
}

// ---- what an operator asks of its input: keys of la or lb bases, every extension of ext_len bases ------------------------------------
__global__ __launch_bounds__(256) void k_rd_check(const DynView v, int64_t n, int la, int lb, int ext_len, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int len = (int)v.key_len[i];
    uint32_t bad = (len != la && len != lb) ? (uint32_t)RD_BAD_LEN : 0u;
    if (v.ext_len[i] != ext_len) bad |= RD_BAD_EXT;
    if (bad) atomicOr(&flags->bad, bad);
}

// ---- step 3: LeftLongerToShorterComparisonPreparation -- key' = the first len - 1 bases REVERSED, extension' = the last base, marker 1
__global__ __launch_bounds__(256) void k_rd_left_prep(const DynView v, int64_t n, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[n] = n;
    if (i >= n) return;
    const int len = (int)v.key_len[i];
    const Pk4 w = pk_load(v.key, i);
    pk_store(o.key, i, pk_reverse(w, len - 1));
    o.key_len[i] = (uint8_t)(len - 1);
    o.ext[i] = pk_base(w, len - 1) << 62;
    o.ext_off[i] = i;
    o.ext_len[i] = 1;
    o.marker[i] = 1; o.left[i] = v.left[i]; o.right[i] = v.right[i];
}
// ---- step 6: RightLongerToShorterComparisonAndNeutralizationPreparation -- the key reversed back, joined with the extension (behind
// it for marker 1, ahead of it otherwise), the first base cut off as the new extension, marker 2
__global__ __launch_bounds__(256) void k_rd_right_prep(const DynView v, int64_t n, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[n] = n;
    if (i >= n) return;
    const int len = (int)v.key_len[i];
    const Pk4 w = pk_reverse(pk_load(v.key, i), len);
    const uint64_t e = v.ext[v.ext_off[i]] >> 62;
    Pk4 c;                                                           // len + 1 <= 125 bases
    if (v.marker[i] == 1) { c = w; pk_or(c, len >> 5, pk_at(e, len)); }
    else c = Pk4{(w.w0 >> 2) | (e << 62), (w.w1 >> 2) | (w.w0 << 62), (w.w2 >> 2) | (w.w1 << 62), (w.w3 >> 2) | (w.w2 << 62)};
    pk_store(o.key, i, pk_keep4(pk_shl(c, 1), len));
    o.key_len[i] = (uint8_t)len;
    o.ext[i] = c.w0 & (3ull << 62);
    o.ext_off[i] = i;
    o.ext_len[i] = 1;
    o.marker[i] = 2; o.left[i] = v.left[i]; o.right[i] = v.right[i];
}

// ---- steps 5 and 8: the two window adjustments ----------------------------------------------------------------------------------------
// the first and the last row of every partition that has rows (info is zeroed before)
__global__ void k_rd_marks(const int64_t *__restrict__ ps, int P, uint32_t *__restrict__ info) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= P || ps[p] >= ps[p + 1]) return;
    atomicOr(info + ps[p], (uint32_t)RD_START);
    atomicOr(info + ps[p + 1] - 1, (uint32_t)RD_END);
}
// One thread per row: rows i - 2, i - 1, i into the nine bits (a row that does not exist leaves its bits 0), the row's map
template <bool RIGHT>
__global__ __launch_bounds__(256) void k_rd_window(const DynView v, int64_t n, int short_len, uint32_t *__restrict__ info, uint8_t *__restrict__ maps) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int lc = (int)v.key_len[i];
    const Pk4 c = pk_load(v.key, i);
    const uint64_t ec = v.ext[v.ext_off[i]] >> 62;
    unsigned in = lc == short_len ? RFX_FSM_SC : 0;
    if (i >= 1) {
        const int lb = (int)v.key_len[i - 1];
        const Pk4 b = pk_load(v.key, i - 1);
        const uint64_t eb = v.ext[v.ext_off[i - 1]] >> 62;
        in |= (lb == short_len ? RFX_FSM_SB : 0) | (pk_prefix(b, lb, c, lc) ? RFX_FSM_PBC : 0) | (eb == ec ? RFX_FSM_EBC : 0);
        if (i >= 2) {
            const int la = (int)v.key_len[i - 2];
            const Pk4 a = pk_load(v.key, i - 2);
            const uint64_t ea = v.ext[v.ext_off[i - 2]] >> 62;
            in |= (la == short_len ? RFX_FSM_SA : 0) | (pk_prefix(a, la, b, lb) ? RFX_FSM_PAB : 0) | (pk_prefix(a, la, c, lc) ? RFX_FSM_PAC : 0) |
                  (ea == eb ? RFX_FSM_EAB : 0) | (ea == ec ? RFX_FSM_EAC : 0);
        }
    }
    const uint32_t marks = info[i];
    info[i] = marks | (in << RD_IN_SHIFT);
    maps[i] = (uint8_t)rfx_fsm_map((marks & RD_START) != 0, i >= 2 ? rfx_fsm_window(RIGHT, in).next : 0u);
}
// the inclusive scan of 256 maps under composition (first the earlier row's); sh: 256 words of LDS
__device__ __forceinline__ unsigned rd_block_scan(unsigned m, unsigned *sh) {
    const int t = (int)threadIdx.x;
    sh[t] = m;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned x = t >= d ? rfx_fsm_compose(sh[t - d], sh[t]) : sh[t];
        __syncthreads();
        sh[t] = x;
        __syncthreads();
    }
    return sh[t];
}
__global__ __launch_bounds__(256) void k_rd_scan_reduce(const uint8_t *__restrict__ maps, int64_t n, uint8_t *__restrict__ agg) {
    __shared__ unsigned sh[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned inc = rd_block_scan(i < n ? (unsigned)maps[i] : RFX_FSM_IDENTITY, sh);
    if (threadIdx.x == 255) agg[blockIdx.x] = (uint8_t)inc;
}
// ONE block: agg[b] := the composite of the blocks before b.  A thread composes its stretch of ceil(nb / 256) aggregates, the
// block scans the 256 stretch composites, the thread rewrites its stretch
__global__ __launch_bounds__(256) void k_rd_scan_aggs(uint8_t *__restrict__ agg, int64_t nb) {
    __shared__ unsigned sh[256];
    const int64_t per = (nb + 255) / 256, b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    unsigned m = RFX_FSM_IDENTITY;
    for (int64_t b = b0; b < b1; b++) m = rfx_fsm_compose(m, (unsigned)agg[b]);
    rd_block_scan(m, sh);
    unsigned run = threadIdx.x ? sh[threadIdx.x - 1] : RFX_FSM_IDENTITY;
    for (int64_t b = b0; b < b1; b++) {
        const unsigned t = (unsigned)agg[b];
        agg[b] = (uint8_t)run;
        run = rfx_fsm_compose(run, t);
    }
}
// what row i writes, given the state ahead of it: its window's step, its flush's step, or the one pending row
struct RdSteps { rfx_fsm_step w, f; bool one; };
template <bool RIGHT>
__device__ __forceinline__ RdSteps rd_steps(uint32_t info, unsigned state, int64_t i) {
    const unsigned in = (info >> RD_IN_SHIFT) & 0x1FFu;
    unsigned s = (info & RD_START) ? 0u : state;
    if ((int64_t)s > i) s = (unsigned)i;                             // (never more rows pending than there are rows before this one)
    RdSteps r{rfx_fsm_step{s + 1, 0u, 0u}, rfx_fsm_step{0u, 0u, 0u}, false};
    if (s == 2) r.w = rfx_fsm_window(RIGHT, in);
    if (info & RD_END) {
        // the pending pair is rows i - 1, i: their bits are the window's b, c
        if (r.w.next == 2) r.f = rfx_fsm_flush(RIGHT, ((in & RFX_FSM_SB) ? RFX_FSM_SA : 0) | ((in & RFX_FSM_SC) ? RFX_FSM_SB : 0) | ((in & RFX_FSM_PBC) ? RFX_FSM_PAB : 0));
        else if (r.w.next == 1) r.one = true;
    }
    return r;
}
template <bool RIGHT>
__global__ __launch_bounds__(256) void k_rd_scan_apply(const uint8_t *__restrict__ maps, const uint8_t *__restrict__ agg, int64_t n,
                                                       uint32_t *__restrict__ info, uint32_t *__restrict__ cnt) {
    __shared__ unsigned sh[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    rd_block_scan(i < n ? (unsigned)maps[i] : RFX_FSM_IDENTITY, sh);
    const unsigned before = rfx_fsm_compose((unsigned)agg[blockIdx.x], threadIdx.x ? sh[threadIdx.x - 1] : RFX_FSM_IDENTITY);
    if (i >= n) return;
    const unsigned state = rfx_fsm_apply(before, 0u);
    const uint32_t w = info[i];
    const RdSteps st = rd_steps<RIGHT>(w, state, i);
    info[i] = w | (state << RD_STATE_SHIFT);
    cnt[i] = rfx_fsm_popcount3(st.w.emit) + rfx_fsm_popcount3(st.f.emit) + (st.one ? 1u : 0u);
}
// record q of the output := row j, or row j edited from row src (src >= 0): the other's extension, its own marker set to -1
// where the other's is negative and its own is not -- the right marker in the left adjustment, the left one in the right
template <bool RIGHT>
__device__ __forceinline__ void rd_put(const DynView &v, const DynOut &o, int64_t q, int64_t j, int64_t src) {
    pk_store(o.key, q, pk_load(v.key, j));
    o.key_len[q] = v.key_len[j];
    o.ext[q] = v.ext[v.ext_off[src >= 0 ? src : j]] & (3ull << 62);
    o.ext_off[q] = q;
    o.ext_len[q] = 1;
    int l = v.left[j], r = v.right[j];
    if (src >= 0) { if (RIGHT) l = rfx_fsm_edit_marker(l, v.left[src]); else r = rfx_fsm_edit_marker(r, v.right[src]); }
    o.marker[q] = v.marker[j]; o.left[q] = l; o.right[q] = r;
}
// rows first .. first + 2 under a step's emit bits and edit
template <bool RIGHT>
__device__ __forceinline__ int64_t rd_put_step(const DynView &v, const DynOut &o, int64_t q, int64_t first, const rfx_fsm_step &st) {
    if (st.emit & 1u) rd_put<RIGHT>(v, o, q++, first, st.edit == 1 ? first + 1 : -1);
    if (st.emit & 2u) rd_put<RIGHT>(v, o, q++, first + 1, st.edit == 2 ? first : -1);
    if (st.emit & 4u) rd_put<RIGHT>(v, o, q++, first + 2, -1);
    return q;
}
template <bool RIGHT>
__global__ __launch_bounds__(256) void k_rd_emit(const DynView v, int64_t n, const uint32_t *__restrict__ info, const uint64_t *__restrict__ off,
                                                 const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[off[n]] = (int64_t)off[n];
    if (i >= n) return;
    const uint32_t w = info[i];
    const RdSteps st = rd_steps<RIGHT>(w, (w >> RD_STATE_SHIFT) & 3u, i);
    int64_t q = (int64_t)off[i];
    if (st.w.emit) q = rd_put_step<RIGHT>(v, o, q, i - 2, st.w);      // (emit != 0 only from state 2: i >= 2 in its partition)
    if (st.f.emit) q = rd_put_step<RIGHT>(v, o, q, i - 1, st.f);      // (a flush of two: i >= 1; its emit has no third bit)
    if (st.one) rd_put<RIGHT>(v, o, q, i, -1);
}

// ---- step 11: ShorterKmerNeutralization -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rd_nt_long(const DynView v, int64_t n, int k2, uint32_t *__restrict__ isl) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) isl[i] = (int)v.key_len[i] == k2 ? 1u : 0u;
}
// a short row: near[i] = the nearest long row before it in its partition (-1: none), brk[i] = 1 when there is none or the row is
// no prefix of it -- the row breaks the stretch of dropped rows behind that long row
__global__ __launch_bounds__(256) void k_rd_nt_break(const DynView v, int64_t n, const uint32_t *__restrict__ isl, const uint64_t *__restrict__ lrank,
                                                     const int64_t *__restrict__ lidx, const int64_t *__restrict__ ps, int P,
                                                     int64_t *__restrict__ near, uint32_t *__restrict__ brk) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t j = -1;
    uint32_t b = 0;
    if (!isl[i]) {
        if (lrank[i] > 0) j = lidx[lrank[i] - 1];
        if (j < ps[rd_part_of(ps, P, i)]) j = -1;
        b = (j < 0 || !pk_prefix(pk_load(v.key, i), (int)v.key_len[i], pk_load(v.key, j), (int)v.key_len[j])) ? 1u : 0u;
    }
    near[i] = j;
    brk[i] = b;
}
__global__ __launch_bounds__(256) void k_rd_nt_keep(const DynView v, int64_t n, const uint32_t *__restrict__ isl, const int64_t *__restrict__ near,
                                                    const uint64_t *__restrict__ cbrk, const int64_t *__restrict__ ps, int P, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t kp = 1;
    if (!isl[i]) {
        const int64_t j = near[i];
        const bool dropped = j >= 0 && cbrk[i + 1] == cbrk[j + 1];    // no row in (j, i] breaks the stretch
        const int64_t end = ps[rd_part_of(ps, P, i) + 1];
        const bool replaced = i + 1 < end && isl[i + 1] &&
                              pk_prefix(pk_load(v.key, i), (int)v.key_len[i], pk_load(v.key, i + 1), (int)v.key_len[i + 1]);
        kp = (dropped || replaced) ? 0u : 1u;
    }
    keep[i] = kp;
}
// the kept records of a full k-mer set (no extension words), in order
__global__ __launch_bounds__(256) void k_rd_compact(const DynView v, int64_t n, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank,
                                                    const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[rank[n]] = 0;
    if (i >= n || !keep[i]) return;
    const int64_t q = (int64_t)rank[i];
    pk_store(o.key, q, pk_load(v.key, i));
    o.key_len[q] = v.key_len[i];
    o.ext_off[q] = 0;
    o.ext_len[q] = 0;
    o.marker[q] = v.marker[i]; o.left[q] = v.left[i]; o.right[q] = v.right[i];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static int rd_params(rfx_ctx *ctx, const rfx_reduce_params *p, RdParams *o) {
    if (!p) return RFX_E_ARG;
    if (p->k1 < 8 || p->k1 >= p->k2 || p->k2 > 124) { ctx->last_error = "k-mer reduction: k1 and k2 must be 8 <= k1 < k2 <= 124"; return RFX_E_ARG; }
    if (p->max_k < p->k2 || p->max_k + 3 > PK_CLAMP) { ctx->last_error = "k-mer reduction: max_k below k2 or out of range"; return RFX_E_ARG; }
    *o = RdParams{p->k1, p->k2};
    return RFX_OK;
}
static int rd_bad(rfx_ctx *ctx, uint32_t bad) {
    ctx->last_error = bad & RD_BAD_OFFSETS ? "k-mer reduction: row offsets that run backwards"
                    : bad & RD_BAD_COMMA   ? "k-mer reduction: a row without a comma"
                    : bad & RD_BAD_LEN     ? "k-mer reduction: a key whose length is neither of the two the operator expects"
                                           : "k-mer reduction: a record whose extension is not what the operator expects";
    return RFX_E_ARG;
}
static int rd_check(rfx_ctx *ctx, const DynDev &in, int la, int lb, int ext_len) {
    DevBuf flags;
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_rd_check, in.n, dyn_view(in), in.n, la, lb, ext_len, flags.as<CallFlags>());
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));
    return f.bad ? rd_bad(ctx, f.bad) : RFX_OK;
}
// one text's rows into records [base, base + kept) of d (allocated by the caller for n rows more)
struct RdBin { DevBuf len, keep, slot, kbeg, mlr; int64_t kept = 0; };
static int rd_bin_sizes(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, const RdParams &prm, RdBin &b) {
    b.kept = 0;
    if (n == 0) return RFX_OK;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "k-mer reduction: 2^31 rows or more"; return RFX_E_LIMIT; }
    DevBuf flags;
    RFX_ALLOC(b.len, uint32_t, n); RFX_ALLOC(b.keep, uint32_t, n);
    RFX_ALLOC(b.slot, uint64_t, n + 1); RFX_ALLOC(b.kbeg, int64_t, n);
    RFX_ALLOC(b.mlr, int32_t, 3 * n);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_rd_bin_sizes, n, d_text, d_row_off, n, prm, b.len.as<uint32_t>(), b.kbeg.as<int64_t>(), b.mlr.as<int32_t>(),
                 flags.as<CallFlags>());
    RFX_LAUNCH_N(k_rd_bin_flag, n, b.len.as<uint32_t>(), n, b.keep.as<uint32_t>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, b.keep.as<uint32_t>(), b.slot.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, b.slot.as<uint64_t>() + n, nullptr, nullptr, &f));
    if (f.bad) return rd_bad(ctx, f.bad);
    b.kept = (int64_t)f.total[0];
    return RFX_OK;
}
static int rd_bin_emit(rfx_ctx *ctx, const char *d_text, int64_t n, const RdBin &b, int64_t base, DynDev &d) {
    if (n == 0 || b.kept == 0) return RFX_OK;
    RFX_LAUNCH_N(k_rd_bin_emit, n, d_text, n, b.len.as<uint32_t>(), b.slot.as<uint64_t>(),
                 b.kbeg.as<int64_t>(), b.mlr.as<int32_t>(), base, dyn_out(d));
    return RFX_OK;
}
// steps 1-2: both texts -> one set of full k-mer records, the longer input's first
static int rd_union(rfx_ctx *ctx, const char *d_ts, const int64_t *d_os, int64_t ns, const char *d_tl, const int64_t *d_ol, int64_t nl,
                    const RdParams &prm, DynDev &d) {
    RdBin bs, bl;
    RFX_TRY(rd_bin_sizes(ctx, d_tl, d_ol, nl, prm, bl));
    RFX_TRY(rd_bin_sizes(ctx, d_ts, d_os, ns, prm, bs));
    const int64_t n = bl.kept + bs.kept;
    if (n == 0) return dyn_empty(ctx, d);
    RFX_TRY(dyn_alloc(ctx, d, n, 0));
    RFX_HIP(hipMemsetAsync(d.ext_off.as<int64_t>() + n, 0, 8, ctx->stream));
    RFX_TRY(rd_bin_emit(ctx, d_tl, nl, bl, 0, d));
    return rd_bin_emit(ctx, d_ts, ns, bs, bl.kept, d);
}
// step 3 (right == false, on full k-mers) / step 6 (right == true, on sub-k-mers)
static int rd_prepare(rfx_ctx *ctx, bool right, const DynDev &in, const RdParams &prm, DynDev &out) {
    const int64_t n = in.n;
    if (n == 0) return dyn_empty(ctx, out);
    RFX_TRY(right ? rd_check(ctx, in, prm.k1 - 1, prm.k2 - 1, 1) : rd_check(ctx, in, prm.k1, prm.k2, 0));
    RFX_TRY(dyn_alloc(ctx, out, n, n));
    if (right) RFX_LAUNCH_N(k_rd_right_prep, n, dyn_view(in), n, dyn_out(out));
    else RFX_LAUNCH_N(k_rd_left_prep, n, dyn_view(in), n, dyn_out(out));
    return RFX_OK;
}
// steps 5 and 8 over a sorted set cut into P partitions
template <bool RIGHT>
static int rd_adjust_t(rfx_ctx *ctx, const DynDev &in, const int64_t *d_ps, int P, const RdParams &prm, DynDev &out, DevBuf &out_ps) {
    const int64_t n = in.n;
    RFX_TRY(part_starts_alloc(ctx, out_ps, P, n == 0));
    if (n == 0) return dyn_empty(ctx, out);
    RFX_TRY(check_part_starts(ctx, d_ps, P, n, "k-mer reduction"));
    RFX_TRY(rd_check(ctx, in, prm.k1 - 1, prm.k2 - 1, 1));
    const int64_t nb = ceil_div(n, 256);
    DevBuf info, maps, agg, cnt, off;
    RFX_ALLOC(info, uint32_t, n); RFX_HIP(maps.alloc((size_t)n, ctx->stream)); RFX_HIP(agg.alloc((size_t)nb, ctx->stream));
    RFX_ALLOC(cnt, uint32_t, n); RFX_ALLOC(off, uint64_t, n + 1);
    RFX_HIP(hipMemsetAsync(info.p, 0, (size_t)n * 4, ctx->stream));
    const DynView v = dyn_view(in);
    RFX_LAUNCH(k_rd_marks, dim3(1), dim3(64), 0, d_ps, P, info.as<uint32_t>());
    RFX_LAUNCH_N(k_rd_window<RIGHT>, n, v, n, prm.k1 - 1, info.as<uint32_t>(), maps.as<uint8_t>());
    RFX_LAUNCH_N(k_rd_scan_reduce, n, maps.as<uint8_t>(), n, agg.as<uint8_t>());
    RFX_LAUNCH(k_rd_scan_aggs, dim3(1), dim3(256), 0, agg.as<uint8_t>(), nb);
    RFX_LAUNCH_N(k_rd_scan_apply<RIGHT>, n, maps.as<uint8_t>(), agg.as<uint8_t>(), n, info.as<uint32_t>(),
                 cnt.as<uint32_t>());
    int64_t total = 0;
    RFX_TRY(scan_keep(ctx, cnt.as<uint32_t>(), n, off.as<uint64_t>(), &total));
    if (total > n) { ctx->last_error = "k-mer reduction: an adjustment would write more rows than it read"; return RFX_E_STATE; }
    RFX_TRY(dyn_alloc(ctx, out, total, total));
    RFX_LAUNCH_N(k_rd_emit<RIGHT>, n, v, n, info.as<uint32_t>(), off.as<uint64_t>(), dyn_out(out));
    return out_part_starts(ctx, d_ps, P, off.as<uint64_t>(), out_ps.as<int64_t>());
}
static int rd_adjust(rfx_ctx *ctx, bool right, const DynDev &in, const int64_t *d_ps, int P, const RdParams &prm, DynDev &out, DevBuf &out_ps) {
    return right ? rd_adjust_t<true>(ctx, in, d_ps, P, prm, out, out_ps) : rd_adjust_t<false>(ctx, in, d_ps, P, prm, out, out_ps);
}
// step 11 over a sorted set of full k-mers cut into P partitions
static int rd_neutralize(rfx_ctx *ctx, const DynDev &in, const int64_t *d_ps, int P, const RdParams &prm, DynDev &out, DevBuf &out_ps) {
    const int64_t n = in.n;
    RFX_TRY(part_starts_alloc(ctx, out_ps, P, n == 0));
    if (n == 0) return dyn_empty(ctx, out);
    RFX_TRY(check_part_starts(ctx, d_ps, P, n, "k-mer reduction"));
    RFX_TRY(rd_check(ctx, in, prm.k1, prm.k2, 0));
    DevBuf isl, lrank, lidx, near, brk, cbrk, keep, rank;
    RFX_ALLOC(isl, uint32_t, n); RFX_ALLOC(lrank, uint64_t, n + 1); RFX_ALLOC(lidx, int64_t, n);
    RFX_ALLOC(near, int64_t, n); RFX_ALLOC(brk, uint32_t, n); RFX_ALLOC(cbrk, uint64_t, n + 1);
    RFX_ALLOC(keep, uint32_t, n); RFX_ALLOC(rank, uint64_t, n + 1);
    const DynView v = dyn_view(in);
    RFX_LAUNCH_N(k_rd_nt_long, n, v, n, prm.k2, isl.as<uint32_t>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, isl.as<uint32_t>(), lrank.as<uint64_t>(), n));
    RFX_TRY(index_kept(ctx, isl.as<uint32_t>(), lrank.as<uint64_t>(), n, lidx.as<int64_t>()));
    RFX_LAUNCH_N(k_rd_nt_break, n, v, n, isl.as<uint32_t>(), lrank.as<uint64_t>(),
                 lidx.as<int64_t>(), d_ps, P, near.as<int64_t>(), brk.as<uint32_t>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, brk.as<uint32_t>(), cbrk.as<uint64_t>(), n));
    RFX_LAUNCH_N(k_rd_nt_keep, n, v, n, isl.as<uint32_t>(), near.as<int64_t>(),
                 cbrk.as<uint64_t>(), d_ps, P, keep.as<uint32_t>());
    int64_t total = 0;
    RFX_TRY(scan_keep(ctx, keep.as<uint32_t>(), n, rank.as<uint64_t>(), &total));
    RFX_TRY(dyn_alloc(ctx, out, total, 0));
    RFX_LAUNCH_N(k_rd_compact, n, v, n, keep.as<uint32_t>(), rank.as<uint64_t>(), dyn_out(out));
    return out_part_starts(ctx, d_ps, P, rank.as<uint64_t>(), out_ps.as<int64_t>());
}

// steps 1-2 from two packed sets of full k-mers: the long set's records of k2 bases, then the short set's of k1 bases -- the set
// rd_union makes of ks_set_to_text(lng, k2) and ks_set_to_text(sht, k1)
static int rd_union_packed(rfx_ctx *ctx, const DynDev &sht, const DynDev &lng, const RdParams &prm, DynDev &d) {
    if (sht.n >= ((int64_t)1 << 31) || lng.n >= ((int64_t)1 << 31)) { ctx->last_error = "k-mer reduction: 2^31 rows or more"; return RFX_E_LIMIT; }
    DevBuf ks, rs, kl, rl;
    int64_t ms = 0, ml = 0;
    RFX_TRY(ks_select_length(ctx, lng, prm.k2, kl, rl, &ml));
    RFX_TRY(ks_select_length(ctx, sht, prm.k1, ks, rs, &ms));
    const int64_t n = ml + ms;
    if (n == 0) return dyn_empty(ctx, d);
    RFX_TRY(dyn_alloc(ctx, d, n, 0));
    RFX_HIP(hipMemsetAsync(d.ext_off.as<int64_t>() + n, 0, 8, ctx->stream));
    if (ml) RFX_LAUNCH_N(k_rd_pk_emit, lng.n, dyn_view(lng), lng.n, kl.as<uint32_t>(), rl.as<uint64_t>(), (int64_t)0, dyn_out(d));
    if (ms) RFX_LAUNCH_N(k_rd_pk_emit, sht.n, dyn_view(sht), sht.n, ks.as<uint32_t>(), rs.as<uint64_t>(), ml, dyn_out(d));
    return RFX_OK;
}

// the driver behind either union (a is used up); the set stays in HBM between the operators
static int rd_run_set(rfx_ctx *ctx, DynDev &a, int P, const RdParams &prm, DynDev &out) {
    DynDev b;
    DevBuf ps, ops;
    uint32_t lmin = 0;
    RFX_TRY(rd_prepare(ctx, false, a, prm, b));
    RFX_TRY(dyn_sort(ctx, b, P, a, ps, &lmin));
    RFX_TRY(rd_adjust(ctx, false, a, ps.as<int64_t>(), P, prm, b, ops));
    RFX_TRY(rd_prepare(ctx, true, b, prm, a));
    RFX_TRY(dyn_sort(ctx, a, P, b, ps, &lmin));
    RFX_TRY(rd_adjust(ctx, true, b, ps.as<int64_t>(), P, prm, a, ops));
    RFX_TRY(ks_set_full_kmers(ctx, a, b));
    RFX_TRY(dyn_sort(ctx, b, P, a, ps, &lmin));
    return rd_neutralize(ctx, a, ps.as<int64_t>(), P, prm, out, ops);
}
static int rd_run(rfx_ctx *ctx, const char *d_ts, const int64_t *d_os, int64_t ns, const char *d_tl, const int64_t *d_ol, int64_t nl, int P,
                  const RdParams &prm, DynDev &out) {
    DynDev a;
    RFX_TRY(rd_union(ctx, d_ts, d_os, ns, d_tl, d_ol, nl, prm, a));
    return rd_run_set(ctx, a, P, prm, out);
}

// ---- the driver from reads (rfx_dev_reduce_reads): Pipelines.reflexivDSDynamicReductionPipe on the read store ----
static bool rr_k_ok(int k) { return k >= 8 && k <= 124 && k != 32 && k != 63 && k != 94 && k != 64 && k != 96; }
// E of every k of the list (Pipelines.java:1412-1416, :1489-1493: the reference mutates param, so the value stays): sorting the first k
// sets 3 min_cov iff (k >= 61 and the second k < 81) or k >= 81, sorting a later k iff k >= 61
static std::vector<int> rr_error_cov(const int *klist, int n_k, const rfx_reduce_reads_params &p) {
    std::vector<int> out((size_t)n_k);
    int E = p.min_error_cov;
    for (int i = 0; i < n_k; i++) {
        const int k = klist[i];
        if (i == 0 ? ((k >= 61 && klist[1] < 81) || k >= 81) : k >= 61) E = 3 * p.min_cov;
        out[(size_t)i] = E;
    }
    return out;
}
static rfx_ksort_params rr_ksort_params(const int *klist, int n_k, int i, int E, const rfx_reduce_reads_params &p) {
    return rfx_ksort_params{klist[i], klist[n_k - 1], E, p.max_cov, p.bubble, p.min_repeat_fold};
}
static int rr_args(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_read_len, const int *klist, int n_k,
                   const rfx_reduce_reads_params *p) {
    if (!klist || !p || n_reads < 0 || (n_reads > 0 && (!d_words || !d_read_len)) || wpr < 1 || max_read_len < 0 || (int64_t)wpr * 32 < max_read_len) return RFX_E_ARG;
    if (n_k < 2 || n_k > 16) { ctx->last_error = "reduction from reads: the k list must hold 2..16 values"; return RFX_E_ARG; }
    for (int i = 0; i < n_k; i++) {
        if (!rr_k_ok(klist[i])) { ctx->last_error = "reduction from reads: a k outside 8..124, or 32, 63, 94 (the sorter refuses them), or 64, 96 (the counter does)"; return RFX_E_ARG; }
        if (i > 0 && klist[i] <= klist[i - 1]) { ctx->last_error = "reduction from reads: the k list is not strictly ascending"; return RFX_E_ARG; }
        if (p->sensitive && klist[i] <= 31 && wpr > 937) { ctx->last_error = "reduction from reads: sensitive mode takes reads of at most 937 words"; return RFX_E_ARG; }
    }
    if (!parts_ok(p->P)) { ctx->last_error = "reduction from reads: P outside 1..63"; return RFX_E_ARG; }
    if (p->front_clip < 0 || p->end_clip < 0 || p->max_cov < 0 || p->min_cov < 0 || p->min_cov > 10000 || (p->bubble != 0 && p->bubble != 1) ||
        (p->sensitive != 0 && p->sensitive != 1)) { ctx->last_error = "reduction from reads: a clip, a coverage or a switch out of range"; return RFX_E_ARG; }
    // what the sorter itself refuses, for every k with the E the rule gives it, ahead of any work
    const std::vector<int> E = rr_error_cov(klist, n_k, *p);
    for (int i = 0; i < n_k; i++) {
        const rfx_ksort_params kp = rr_ksort_params(klist, n_k, i, E[(size_t)i], *p);
        RFX_TRY(ks_params_check(ctx, &kp));
    }
    return RFX_OK;
}
static double rr_now_ms() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }
// one k: count (and the mercy k-mers of a k <= 31 in sensitive mode), then steps 1-8 of the sorter on the counter's arrays
static int rr_sorted(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_read_len, int k,
                     const rfx_reduce_reads_params &p, const rfx_ksort_params &kp, DynDev &out) {
    const int W = k / 32 + 1, cb = k <= 31 ? 4 : 8;
    const double t_enter = rr_now_ms();
    // every survivor has min_cov instances or more, and a read has at most len - k + 1 windows: that bound always holds, but at depth
    // it is many times the survivors (12 x at depth 30) and the scratch is the call's largest allocation -- so an eighth of it first,
    // and where that is short the counter says what it needs and one more count (milliseconds) follows
    const int64_t inst = n_reads * (int64_t)std::max(max_read_len - k + 1, 0);
    int64_t cap = inst / std::max(p.min_cov, 1) / 8 + 1024, n = 0, distinct = 0, instances = 0;
    DevBuf keys, counts, extra;
    for (int attempt = 0;; attempt++) {
        RFX_ALLOC(keys, uint64_t, cap * W); RFX_HIP(counts.alloc((size_t)cap * cb, ctx->stream));
        const int st = k <= 31 ? rfx_dev_count_reads_ragged(ctx, d_words, d_read_len, n_reads, wpr, max_read_len, k, p.front_clip, p.end_clip, p.min_cov, p.max_cov,
                                                            RFX_TWIN_DS, keys.as<uint64_t>(), counts.as<int32_t>(), cap, &n, &distinct, &instances)
                               : rfx_dev_count_reads_ragged_w(ctx, d_words, d_read_len, n_reads, wpr, max_read_len, k, p.front_clip, p.end_clip, p.min_cov, p.max_cov,
                                                              keys.as<uint64_t>(), counts.as<int64_t>(), cap, &n, &distinct, &instances);
        if (st == RFX_E_CAP && attempt == 0) { cap = n > cap ? n : inst / std::max(p.min_cov, 1) + 1; continue; }
        if (st == RFX_E_CAP) { ctx->last_error = "reduction from reads: the counter's output did not fit the capacity it asked for"; return RFX_E_STATE; }
        RFX_TRY(st);
        break;
    }
    const double t_counted = rr_now_ms();
    int64_t n_extra = 0;
    if (p.sensitive && k <= 31) {
        const int st = rfx_dev_mercy_kmers(ctx, keys.as<uint64_t>(), n, d_words, d_read_len, n_reads, wpr, k, p.front_clip, p.end_clip, nullptr, 0, &n_extra);
        if (st != RFX_E_CAP) RFX_TRY(st);
        if (n_extra > 0) {
            RFX_ALLOC(extra, uint64_t, n_extra);
            RFX_TRY(rfx_dev_mercy_kmers(ctx, keys.as<uint64_t>(), n, d_words, d_read_len, n_reads, wpr, k, p.front_clip, p.end_clip, extra.as<uint64_t>(), n_extra,
                                        &n_extra));
        }
    }
    const double t_sort = rr_now_ms();
    const int st = ks_run_counts(ctx, keys.as<uint64_t>(), counts.p, cb, n, extra.as<uint64_t>(), n_extra, &kp, out);
    if (getenv("RFX_REDUCE_TRACE"))
        fprintf(stderr, "reduce_reads: k %d: scratch + count %.1f ms (%lld rows of a capacity of %lld), mercy %.1f ms, sort %.1f ms\n", k, t_counted - t_enter,
                (long long)n, (long long)cap, t_sort - t_counted, rr_now_ms() - t_sort);
    return st;
}
// a pair's final set, once the next pair has consumed it, cut down to its records of len bases (k_rd_pk_emit again: what it does to a
// field, rfx_dev_dyn_from_kmers does once more anyway, and the marker is not read there)
static int rr_keep_length(rfx_ctx *ctx, DynDev &d, int len) {
    DevBuf keep, rank;
    int64_t m = 0;
    DynDev half;
    RFX_TRY(ks_select_length(ctx, d, len, keep, rank, &m));
    if (m == 0) RFX_TRY(dyn_empty(ctx, half));
    else {
        RFX_TRY(dyn_alloc(ctx, half, m, 0));
        RFX_HIP(hipMemsetAsync(half.ext_off.as<int64_t>() + m, 0, 8, ctx->stream));
        RFX_LAUNCH_N(k_rd_pk_emit, d.n, dyn_view(d), d.n, keep.as<uint32_t>(), rank.as<uint64_t>(), (int64_t)0, dyn_out(half));
    }
    d = std::move(half);                                                  // (d's old buffers are freed in stream order, behind the launch)
    return RFX_OK;
}
// Every k of the list in order: its sorted set, and from the second k on the reduction of the pair (previous, this), whose short
// input is the pair before's final set as it is.  res[i] = the final set of the pair (k_i, k_i+1): its records of k_i bases are
// Count_<k_i>_reduced (all that is kept of it once the next pair has consumed it), the last one's records of k_last bases
// Count_<k_last>_reduced.  sets[i] = where Count_<k_i>_reduced lies.
// RFX_REDUCE_TRACE (set to anything): one line per k on stderr with the host time of each stage of the driver (every stage returns
// after the stream has drained, so these are the stages' whole times)
static int rr_pairs(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_read_len, const int *klist, int n_k,
                    const rfx_reduce_reads_params &p, std::vector<DynDev> &res, std::vector<const DynDev *> &sets) {
    const std::vector<int> E = rr_error_cov(klist, n_k, p);
    DynDev first;                                                      // the first k's sorted set: the short input of the first pair
    const bool trace = getenv("RFX_REDUCE_TRACE") != nullptr;
    for (int i = 0; i < n_k; i++) {
        const int k = klist[i];
        const rfx_ksort_params kp = rr_ksort_params(klist, n_k, i, E[(size_t)i], p);
        const double t0 = rr_now_ms();
        if (i == 0) {
            RFX_TRY(rr_sorted(ctx, d_words, d_read_len, n_reads, wpr, max_read_len, k, p, kp, first));
            if (trace) fprintf(stderr, "reduce_reads: k %d E %d: count + sort %.1f ms, %lld records\n", k, kp.min_error_cov, rr_now_ms() - t0, (long long)first.n);
            continue;
        }
        DynDev cur, uni;
        RFX_TRY(rr_sorted(ctx, d_words, d_read_len, n_reads, wpr, max_read_len, k, p, kp, cur));
        const double t1 = rr_now_ms();
        const RdParams prm{klist[i - 1], k};
        DynDev &sht = i == 1 ? first : res[(size_t)i - 2];
        RFX_TRY(rd_union_packed(ctx, sht, cur, prm, uni));
        if (i == 1) first = DynDev();                                   // (consumed: the union holds what the pair needs of it)
        else RFX_TRY(rr_keep_length(ctx, res[(size_t)i - 2], klist[i - 2]));   // (what is left of it is Count_<k>_reduced alone)
        const int64_t n_cur = cur.n;
        cur = DynDev();
        const double t2 = rr_now_ms();
        RFX_TRY(rd_run_set(ctx, uni, p.P, prm, res[(size_t)i - 1]));
        if (trace) fprintf(stderr, "reduce_reads: k %d E %d: count + sort %.1f ms, %lld records; union %.1f ms; reduction of (%d, %d) %.1f ms, %lld records\n", k,
                           kp.min_error_cov, t1 - t0, (long long)n_cur, t2 - t1, klist[i - 1], k, rr_now_ms() - t2, (long long)res[(size_t)i - 1].n);
    }
    for (int i = 0; i < n_k; i++) sets[(size_t)i] = &res[(size_t)std::min(i, n_k - 2)];
    return RFX_OK;
}
}  // namespace
// ... for the driver from reads to contigs (rfx_meta.hip): what rfx_dev_reduce_reads checks of its arguments / its body, into a set of
// the library's (per_k: n_k row counts, nullable)
int rfx::rr_check_args(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_read_len, const int *klist, int n_k,
                       const rfx_reduce_reads_params *p) {
    return rr_args(ctx, d_words, d_read_len, n_reads, wpr, max_read_len, klist, n_k, p);
}
int rfx::rr_reduce_set(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_read_len, const int *klist, int n_k,
                       const rfx_reduce_reads_params &p, DynDev &a, int64_t *per_k) {
    if (per_k) for (int i = 0; i < n_k; i++) per_k[i] = 0;
    if (n_reads == 0) return dyn_empty(ctx, a);
    std::vector<DynDev> res((size_t)n_k - 1);
    std::vector<const DynDev *> sets((size_t)n_k);
    RFX_TRY(rr_pairs(ctx, d_words, d_read_len, n_reads, wpr, max_read_len, klist, n_k, p, res, sets));
    RFX_TRY(ks_kmers_to_records(ctx, sets.data(), klist, n_k, a, per_k));
    return sync_checked(ctx);                                           // (the sets go back to the pool here: their last reader is behind us)
}

extern "C" {

void rfx_reduce_reads_default_params(rfx_reduce_reads_params *p) try {
    if (!p) return;
    p->min_cov = 2; p->max_cov = 10000000; p->min_error_cov = 8; p->min_repeat_fold = 1.5; p->bubble = 1; p->sensitive = 0;
    p->front_clip = 0; p->end_clip = 0; p->P = 8;
} RFX_API_CATCH_VOID(nullptr)

int rfx_dev_reduce_reads(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int words_per_read, int max_read_len,
                         const int *klist, int n_k, const rfx_reduce_reads_params *params, rfx_dyn_packed *d_out, int64_t *out_n_per_k) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !out_n_per_k) return RFX_E_ARG;
    RFX_TRY(rr_args(ctx, d_words, d_read_len, n_reads, words_per_read, max_read_len, klist, n_k, params));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    std::vector<int64_t> per_k((size_t)n_k, 0);
    if (n_reads == 0) RFX_TRY(dyn_empty(ctx, a));
    else {
        std::vector<DynDev> res((size_t)n_k - 1);
        std::vector<const DynDev *> sets((size_t)n_k);
        RFX_TRY(rr_pairs(ctx, d_words, d_read_len, n_reads, words_per_read, max_read_len, klist, n_k, *params, res, sets));
        RFX_TRY(ks_kmers_to_records(ctx, sets.data(), klist, n_k, a, per_k.data()));
        RFX_TRY(sync_checked(ctx));                                     // (the sets go back to the pool here: their last reader is behind us)
    }
    RFX_TRY(dyn_store(ctx, a, d_out));                                  // (RFX_E_CAP: n and need_words set, nothing written)
    for (int i = 0; i < n_k; i++) out_n_per_k[i] = per_k[(size_t)i];
    return RFX_OK;
} RFX_API_CATCH(ctx)

// host form: ASCII reads in, the rows of every Count_<k>_reduced out in list order; one upload, one encode, one copy back
int rfx_reduce_reads(rfx_ctx *ctx, const uint8_t *bases, const int64_t *read_off, int64_t n_reads, const int *klist, int n_k,
                     const rfx_reduce_reads_params *params, char *out, int64_t cap, int64_t *out_len, int64_t *out_off) try {
    if (!ctx || !text_rows_ok((const char *)bases, read_off, n_reads) || !text_out_ok(out, cap, out_len) || !out_off) return RFX_E_ARG;
    if (n_reads >= ((int64_t)1 << 31)) { ctx->last_error = "reduction from reads: 2^31 reads or more"; return RFX_E_LIMIT; }
    int64_t longest = 1;
    for (int64_t i = 0; i < n_reads; i++) {
        if (read_off[i + 1] < read_off[i]) return RFX_E_ARG;
        longest = std::max(longest, read_off[i + 1] - read_off[i]);
    }
    if (longest > 32 * (int64_t)30000) { ctx->last_error = "reduction from reads: a read of more than 960000 bases"; return RFX_E_LIMIT; }
    const int wpr = (int)((longest + 31) >> 5);
    // (a device pointer is not needed to check the arguments: any non-null stands in for the read store)
    const uint64_t *probe_w = (const uint64_t *)read_off;
    RFX_TRY(rr_args(ctx, probe_w, (const uint32_t *)read_off, n_reads, wpr, (int)longest, klist, n_k, params));
    RFX_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> offs((size_t)n_k + 1, 0);
    std::vector<DevBuf> text((size_t)n_k);
    if (n_reads > 0) {
        DevBuf d_b, d_ro, d_words, d_len;
        RFX_TRY(dyn_upload_text(ctx, (const char *)bases, read_off, n_reads, d_b, d_ro));
        RFX_ALLOC(d_words, uint64_t, n_reads * wpr); RFX_ALLOC(d_len, uint32_t, n_reads);
        RFX_TRY(encode_reads(ctx, d_b.as<uint8_t>(), d_ro.as<int64_t>(), n_reads, wpr, d_words.as<uint64_t>(), d_len.as<uint32_t>()));
        d_b.release(); d_ro.release();
        std::vector<DynDev> res((size_t)n_k - 1);
        std::vector<const DynDev *> sets((size_t)n_k);
        RFX_TRY(rr_pairs(ctx, d_words.as<uint64_t>(), d_len.as<uint32_t>(), n_reads, wpr, (int)longest, klist, n_k, *params, res, sets));
        for (int i = 0; i < n_k; i++) {
            int64_t total = 0, rows = 0;
            RFX_TRY(ks_set_to_text(ctx, *sets[(size_t)i], klist[i], nullptr, 0, &total, nullptr, &rows, &text[(size_t)i]));
            offs[(size_t)i + 1] = offs[(size_t)i] + total;
        }
    }
    *out_len = offs[(size_t)n_k];
    for (int i = 0; i <= n_k; i++) out_off[i] = offs[(size_t)i];
    if (*out_len > cap) return RFX_E_CAP;                                 // (rfx_reduce_text's rule: the lengths set, nothing written)
    for (int i = 0; i < n_k; i++) {
        const int64_t len = offs[(size_t)i + 1] - offs[(size_t)i];
        if (len > 0) RFX_HIP(hipMemcpyAsync(out + offs[(size_t)i], text[(size_t)i].p, (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
    }
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

void rfx_reduce_default_params(rfx_reduce_params *p, int k1, int k2) try {
    if (!p) return;
    p->k1 = k1; p->k2 = k2; p->max_k = 95 > k2 ? 95 : k2;
} RFX_API_CATCH_VOID(nullptr)

int rfx_dev_reduce_union(rfx_ctx *ctx, const char *d_text_short, const int64_t *d_row_off_short, int64_t n_short, const char *d_text_long,
                         const int64_t *d_row_off_long, int64_t n_long, const rfx_reduce_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text_short, d_row_off_short, n_short) || !text_rows_ok(d_text_long, d_row_off_long, n_long)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(rd_union(ctx, d_text_short, d_row_off_short, n_short, d_text_long, d_row_off_long, n_long, prm, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_left_prepare(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_reduce_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(rd_prepare(ctx, false, a, prm, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_right_prepare(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_reduce_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(rd_prepare(ctx, true, a, prm, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_adjust(rfx_ctx *ctx, int right, const rfx_dyn_packed *d_sorted, const int64_t *d_part_start, int P, const rfx_reduce_params *params,
                          rfx_dyn_packed *d_out, int64_t *d_out_part_start) try {
    if (!ctx || !dyn_packed_ok(d_sorted) || !dyn_packed_out_ok(d_out) || !d_part_start || !d_out_part_start || !parts_ok(P) || (right != 0 && right != 1)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ops;
    RFX_TRY(dyn_borrow(ctx, d_sorted, a));
    RFX_TRY(rd_adjust(ctx, right != 0, a, d_part_start, P, prm, b, ops));
    RFX_TRY(dyn_store(ctx, b, d_out));                                // (both capacities are checked before anything is copied)
    return part_starts_store(ctx, d_out_part_start, ops, P);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_full_kmers(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_reduce_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    if (a.n > 0) RFX_TRY(rd_check(ctx, a, prm.k1 - 1, prm.k2 - 1, 1));
    RFX_TRY(ks_set_full_kmers(ctx, a, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_neutralize(rfx_ctx *ctx, const rfx_dyn_packed *d_sorted, const int64_t *d_part_start, int P, const rfx_reduce_params *params,
                              rfx_dyn_packed *d_out, int64_t *d_out_part_start) try {
    if (!ctx || !dyn_packed_ok(d_sorted) || !dyn_packed_out_ok(d_out) || !d_part_start || !d_out_part_start || !parts_ok(P)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ops;
    RFX_TRY(dyn_borrow(ctx, d_sorted, a));
    RFX_TRY(rd_neutralize(ctx, a, d_part_start, P, prm, b, ops));
    RFX_TRY(dyn_store(ctx, b, d_out));
    return part_starts_store(ctx, d_out_part_start, ops, P);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_run(rfx_ctx *ctx, const char *d_text_short, const int64_t *d_row_off_short, int64_t n_short, const char *d_text_long,
                       const int64_t *d_row_off_long, int64_t n_long, int P, const rfx_reduce_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text_short, d_row_off_short, n_short) || !text_rows_ok(d_text_long, d_row_off_long, n_long) ||
        !parts_ok(P)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(rd_run(ctx, d_text_short, d_row_off_short, n_short, d_text_long, d_row_off_long, n_long, P, prm, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_union_packed(rfx_ctx *ctx, const rfx_dyn_packed *d_short, const rfx_dyn_packed *d_long, const rfx_reduce_params *params,
                                rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_short) || !dyn_packed_ok(d_long) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev s, l, a;
    RFX_TRY(dyn_borrow(ctx, d_short, s));
    RFX_TRY(dyn_borrow(ctx, d_long, l));
    RFX_TRY(rd_union_packed(ctx, s, l, prm, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_reduce_run_packed(rfx_ctx *ctx, const rfx_dyn_packed *d_short, const rfx_dyn_packed *d_long, int P, const rfx_reduce_params *params,
                              rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_short) || !dyn_packed_ok(d_long) || !dyn_packed_out_ok(d_out) || !parts_ok(P)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev s, l, a, b;
    RFX_TRY(dyn_borrow(ctx, d_short, s));
    RFX_TRY(dyn_borrow(ctx, d_long, l));
    RFX_TRY(rd_union_packed(ctx, s, l, prm, a));
    RFX_TRY(rd_run_set(ctx, a, P, prm, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

// two host texts in, two host texts out; everything between packed and in HBM: upload, run, to-text twice, one copy back each
int rfx_reduce_text(rfx_ctx *ctx, const char *text_short, const int64_t *row_off_short, int64_t n_short, const char *text_long,
                    const int64_t *row_off_long, int64_t n_long, int P, const rfx_reduce_params *params, char *out_short, int64_t cap_short,
                    int64_t *out_len_short, char *out_long, int64_t cap_long, int64_t *out_len_long) try {
    if (!ctx || !text_rows_ok(text_short, row_off_short, n_short) || !text_rows_ok(text_long, row_off_long, n_long) || !parts_ok(P) || !out_len_short ||
        !out_len_long || cap_short < 0 || cap_long < 0 || (cap_short > 0 && !out_short) || (cap_long > 0 && !out_long)) return RFX_E_ARG;
    RdParams prm;
    RFX_TRY(rd_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_ts, d_os, d_tl, d_ol, d_o1, d_o2;
    DynDev a;
    int64_t t1 = 0, t2 = 0, rows = 0;
    RFX_TRY(dyn_upload_text(ctx, text_short, row_off_short, n_short, d_ts, d_os));
    RFX_TRY(dyn_upload_text(ctx, text_long, row_off_long, n_long, d_tl, d_ol));
    RFX_TRY(rd_run(ctx, (const char *)d_ts.p, d_os.as<int64_t>(), n_short, (const char *)d_tl.p, d_ol.as<int64_t>(), n_long,
                   P, prm, a));
    RFX_TRY(ks_set_to_text(ctx, a, prm.k1, nullptr, 0, &t1, nullptr, &rows, &d_o1));
    RFX_TRY(ks_set_to_text(ctx, a, prm.k2, nullptr, 0, &t2, nullptr, &rows, &d_o2));
    return text_to_host(ctx, {{d_o1, t1, out_short, cap_short, out_len_short}, {d_o2, t2, out_long, cap_long, out_len_long}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"
