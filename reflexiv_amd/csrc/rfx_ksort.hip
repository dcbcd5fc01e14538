// rfx_ksort.hip -- the k-mer sorting stage (Count_<k>_sorted) on packed record sets that stay in HBM:
// P/ReflexivDSKmerLeftAndRightSorting.java, driver `assemblyFromKmer` :105-243 with param.bubble == true and
// param.minErrorCoverage > 0 -- DynamicKmerBinarizer (:1666-1764), filter(count <= maxKmerCoverage) (:178-184),
// DSKmerReverseComplement (:1569-1664), DSForwardSubKmerExtraction (:906-979), sort("k-1"),
// DSFilterForkSubKmerWithErrorCorrection (:426-624), DSReflectedSubKmerExtractionFromForward (:1096-1179), sort("k-1"),
// DSFilterForkReflectedSubKmerWithErrorCorrection (:693-904), DSSubKmerToFullKmer (:1301-1568) and
// DSBinaryFullKmerArrayToString (:246-354).  It turns the counter's `KMER,count` rows into the `KMER,1|left|right` rows that
// rfx_dyn_binarize form 0 reads.
//
// The record sets are rfx_dyn_packed (rfx_dynamic.hip): four key words per record, 32 bases per word, the first base in the two
// highest bits, every bit past the last base 0 and every unused key word 0 -- every producer here writes those zeros.  Every
// extension of this stage is ONE base at the top of ONE word, so ext_off[i] = i.  The two sorts are rfx_dynamic.hip's
// (dyn_sort, unchanged); the order of the 31-base blocks as signed longs is formed there.
//
// DEVIATION from the reference, stated in the header too: one call handles ONE k.  A row whose k-mer has another length is
// dropped at the binarizer; the reference would carry a row of another LISTED length through both folds (where
// subKmerSlotComparator on block arrays of unequal length is not well defined) and drop it at the output stage.  Its own
// pipeline never writes a mixed file.
//
// Kernels: k_ks_bin_sizes (one thread per row: the cut at the comma, the count, keep or drop), a scan, k_ks_bin_emit (the
// k-mer's words from its letters, the reverse complement word-wise: complement, 2-bit group reversal of the four words, one
// funnel shift); k_kc_keep, a scan, k_kc_emit (the same set straight from the counter's keys and counts, one thread per row and
// orientation: DESIGN.md section 32); k_ks_heads + a scan + k_ks_fold<REFLECTED> (the thread at a run's head walks the run with the reference's
// rules and writes the survivor); k_ks_reflect / k_ks_full (the key shifted by one base across its words, the extension base
// put in at the other end); k_ks_text_sizes + two scans + k_ks_text_offsets + k_ks_text_fill (one thread per 8 output bytes).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

namespace {

#define KS_KW PK_KW

// what is wrong with a call's input (CallFlags::bad)
enum { KS_BAD_OFFSETS = 1, KS_BAD_COMMA = 2, KS_BAD_COUNT = 4, KS_BAD_EXT = 8 };

struct KsParams { int k, M, E, max_cov; double F; };

// (the word forms -- Pk4, pk_shl, pk_keep4, pk_rev2, pk_note_lengths, pk_find -- are rfx_packed_words.h's)

// ---- steps 1-4: DynamicKmerBinarizer, the count filter, DSKmerReverseComplement, DSForwardSubKmerExtraction ---------------------
// One thread per row.  The row ends ahead of its trailing newline; the first ',' cuts it; a leading '(' of the k-mer and a
// trailing ')' of the count are dropped; the count is 1 or more decimal digits (anything else: KS_BAD_COUNT -- the reference
// throws; a sign is refused too), 10 or more of them read as 1,000,000,000.  keep = the k-mer has k letters and count <= max_cov.
__global__ __launch_bounds__(256) void k_ks_bin_sizes(const char *__restrict__ text, const int64_t *__restrict__ row_off, int64_t n, const KsParams prm,
                                                      uint32_t *__restrict__ keep, int64_t *__restrict__ kbeg, int32_t *__restrict__ cnt,
                                                      CallFlags *__restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int64_t b = row_off[r], e = row_off[r + 1];
    uint32_t bad = 0;
    if (e < b || b < 0) { bad |= KS_BAD_OFFSETS; e = b = 0; }
    while (e > b && (text[e - 1] == '\n' || text[e - 1] == '\r')) e--;
    int64_t c = b;
    while (c < e && text[c] != ',') c++;
    uint32_t kp = 0;
    int32_t cv = 0;
    if (c >= e) bad |= bad ? 0 : KS_BAD_COMMA;
    else {
        int64_t kb = b, ce = e;
        if (kb < c && text[kb] == '(') kb++;
        if (ce > c + 1 && text[ce - 1] == ')') ce--;
        const int64_t nd = ce - (c + 1);
        bool digits = nd > 0;
        int64_t v = 0;
        for (int64_t i = c + 1; i < ce; i++) {
            const char ch = text[i];
            if (ch < '0' || ch > '9') { digits = false; break; }
            if (nd < 10) v = v * 10 + (ch - '0');
        }
        if (!digits) bad |= KS_BAD_COUNT;
        if (nd >= 10) v = 1000000000;
        kp = (c - kb == prm.k && v <= prm.max_cov) ? 1u : 0u;
        cv = pk_clamp((int32_t)v);                 // buildingAlongFromThreeInt clamps what it stores
        kbeg[r] = kb;
    }
    keep[r] = bad ? 0u : kp;
    cnt[r] = cv;
    if (bad) atomicOr(&flags->bad, bad);
}
// record q of the binarizers' output from a k-mer w: key = the first k - 1 bases, extension = base k - 1 at the top of one word,
// marker 1 (the sub-k-mer record of the binarizers here and of rfx_dyn_binarize form 0)
__device__ __forceinline__ void ks_emit(const DynOut &o, int64_t q, const Pk4 &w, int k, int32_t l, int32_t r) {
    pk_store(o.key, q, pk_keep4(w, k - 1));
    o.key_len[q] = (uint8_t)(k - 1);
    o.ext[q] = pk_base(w, k - 1) << 62;
    o.ext_off[q] = q;
    o.ext_len[q] = 1;
    o.marker[q] = 1; o.left[q] = l; o.right[q] = r;
}
// One thread per row; a kept row writes records 2 s and 2 s + 1 (s = its rank among the kept rows): the k-mer's and then its
// reverse complement's.
__global__ __launch_bounds__(256) void k_ks_bin_emit(const char *__restrict__ text, int64_t n, const KsParams prm, const uint32_t *__restrict__ keep,
                                                     const uint64_t *__restrict__ slot, const int64_t *__restrict__ kbeg, const int32_t *__restrict__ cnt,
                                                     int64_t n_out, const DynOut o) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0) o.ext_off[n_out] = n_out;
    if (r >= n || !keep[r]) return;
    const int k = prm.k;
    const char *s = text + kbeg[r];
    Pk4 f{0, 0, 0, 0};
    for (int j = 0; j < k; j++) {
        const char ch = s[j];
        pk_or(f, j >> 5, pk_at(pk_code(ch), j));
    }
    const Pk4 rc = pk_revcomp(f, k);
    const int32_t c = cnt[r];
    for (int h = 0; h < 2; h++) ks_emit(o, 2 * (int64_t)slot[r] + h, h ? rc : f, k, c, c);
}

// ---- steps 1-4 straight from the counter's arrays (rfx_dev_ksort_from_counts): no text between the counter and the set ---------------
// n rows of the counter (keys of k / 32 + 1 words a row as rfx_dev_count_reads_ragged / _ragged_w write them, counts of 4 or 8
// bytes), then n_extra keys of the same form whose count is 1 (the mercy k-mers)
struct KcIn { const uint64_t *keys; const void *counts; int64_t n; int count_bytes; const uint64_t *extra; int64_t n_extra; };
__device__ __forceinline__ int64_t kc_count(const KcIn &in, int64_t r) {
    return r >= in.n ? 1 : in.count_bytes == 8 ? static_cast<const int64_t *>(in.counts)[r] : (int64_t)static_cast<const int32_t *>(in.counts)[r];
}
// One thread per row.  The count is read as k_ks_bin_sizes reads its digits (ten or more: 1,000,000,000); keep = it is <= max_cov
// (every key has k bases).  A negative count has no text the binarizer takes: KS_BAD_COUNT.
__global__ __launch_bounds__(256) void k_kc_keep(const KcIn in, const KsParams prm, uint32_t *__restrict__ keep, CallFlags *__restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= in.n + in.n_extra) return;
    const int64_t c = kc_count(in, r);
    keep[r] = (c >= 0 && pk_count_as_text(c) <= (int64_t)prm.max_cov) ? 1u : 0u;
    if (c < 0) atomicOr(&flags->bad, (uint32_t)KS_BAD_COUNT);
}
// One thread per (row, orientation): thread 2 r + h writes record 2 s + h of a kept row (s = its rank among the kept rows), h = 0
// the k-mer's and h = 1 its reverse complement's -- neighbouring threads write neighbouring records of every array.
__global__ __launch_bounds__(256) void k_kc_emit(const KcIn in, const KsParams prm, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ slot,
                                                 int64_t n_out, const DynOut o) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, r = t >> 1;
    if (t == 0) o.ext_off[n_out] = n_out;
    if (r >= in.n + in.n_extra || !keep[r]) return;
    const int k = prm.k, W = (k >> 5) + 1, h = (int)(t & 1);
    const Pk4 f = pk_from_counter(r < in.n ? in.keys + (int64_t)W * r : in.extra + (int64_t)W * (r - in.n), k);
    const int32_t c = pk_clamp((int32_t)pk_count_as_text(kc_count(in, r)));
    ks_emit(o, 2 * (int64_t)slot[r] + h, h ? pk_revcomp(f, k) : f, k, c, c);
}

// ---- full k-mers back to the sub-k-mer records of the dynamic-k passes (rfx_dev_dyn_from_kmers), and the choice by key length ------
// keep = the record's key has len bases
__global__ __launch_bounds__(256) void k_ks_len_keep(const uint8_t *__restrict__ key_len, int64_t n, int len, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keep[i] = (int)key_len[i] == len ? 1u : 0u;
}
// One thread per record of one input set; a kept record writes output record base + (its rank among the kept): what k_ks_text_fill
// prints of it and rfx_dyn_binarize form 0 reads back -- left / right through their decimal text, then clamped; the marker is 1
__global__ __launch_bounds__(256) void k_ks_kmer_emit(const DynView v, int64_t n, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank,
                                                      int64_t base, int64_t n_out, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[n_out] = n_out;
    if (i >= n || !keep[i]) return;
    ks_emit(o, base + (int64_t)rank[i], pk_load(v.key, i), (int)v.key_len[i], pk_clamp(pk_int_as_text(v.left[i])), pk_clamp(pk_int_as_text(v.right[i])));
}

// ---- steps 5 and 7: the two folds over runs of equal keys -----------------------------------------------------------------------
// head[i] = record i opens a run; the set's key lengths and "every extension is one base" go into the flags
__global__ __launch_bounds__(256) void k_ks_heads(const DynView v, int64_t n, uint32_t *__restrict__ head, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    int len = 0;
    if (live) {
        len = (int)v.key_len[i];
        bool h = i == 0;
        if (!h) {
            const uint64_t *x = v.key + KS_KW * i, *y = x - KS_KW;
            h = v.key_len[i - 1] != v.key_len[i] || x[0] != y[0] || x[1] != y[1] || x[2] != y[2] || x[3] != y[3];
        }
        head[i] = h ? 1u : 0u;
        if (v.ext_len[i] != 1) atomicOr(&flags->bad, (uint32_t)KS_BAD_EXT);
    }
    pk_note_lengths(&flags->min_len, &flags->max_len, live, len);
}
// lengths and extension lengths only (reflect, full k-mers): need_ext = every extension must be one base
__global__ __launch_bounds__(256) void k_ks_lengths(const DynView v, int64_t n, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    if (live && v.ext_len[i] != 1) atomicOr(&flags->bad, (uint32_t)KS_BAD_EXT);
    pk_note_lengths(&flags->min_len, &flags->max_len, live, live ? (int)v.key_len[i] : 0);
}
// The thread at a run's head walks the run -- any length, across block edges -- and writes the survivor at the run's rank.
// FORWARD (DSFilterForkSubKmerWithErrorCorrection): state (ext, left, right); extensions compare as signed longs of the block
// form, so G < T < A < C (code ^ 2).  REFLECTED (DSFilterForkReflectedSubKmerWithErrorCorrection): state (ext, left, right) and
// H = HighCoverLastCoverage; extensions compare as base codes.  M = max_k + 3; F is compared in double (the operands are at
// most 30000, the products exact).
template <bool REFLECTED>
__global__ __launch_bounds__(256) void k_ks_fold(const DynView v, int64_t n, const uint32_t *__restrict__ head, const uint64_t *__restrict__ rank,
                                                 const KsParams prm, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[rank[n]] = (int64_t)rank[n];
    if (i >= n || !head[i]) return;
    const int E = prm.E, M = prm.M;
    const double F = prm.F;
    int se = (int)(v.ext[v.ext_off[i]] >> 62), sl, sr, H = v.left[i];
    if (REFLECTED) { sl = -1; sr = v.right[i]; } else { sl = H; sr = -1; }
    for (int64_t j = i + 1; j < n && !head[j]; j++) {
        const int re = (int)(v.ext[v.ext_off[j]] >> 62), rl = v.left[j], rr = v.right[j];
        if (!REFLECTED) {
            const int hi = sl, x = hi == 1 ? -1 : M;
            if (rl > hi) { se = re; sl = rl; sr = (hi <= E && (double)rl >= F * (double)hi) ? -1 : x; }
            else if (rl == hi) { if ((re ^ 2) > (se ^ 2)) se = re; sr = x; }
            else if (rl <= E && (double)hi >= F * (double)rl) sr = -1;
            else { sl = rl; sr = rl == 1 ? -1 : M; }
        } else {
            if (rl > H) { se = re; sl = (H <= E && (double)rl >= F * (double)H) ? -1 : M; sr = rr; H = rl; }
            else if (rl == H) { if (re > se) { se = re; sr = H == 1 ? -1 : rr; } sl = M; }
            else if (rl <= E && (double)H >= F * (double)rl) sl = -1;
            else { sl = M; sr = rl == 1 ? -1 : rr; }
        }
    }
    const int64_t q = (int64_t)rank[i];
    pk_store(o.key, q, pk_load(v.key, i));
    o.key_len[q] = v.key_len[i];
    o.ext[q] = (uint64_t)se << 62;
    o.ext_off[q] = q;
    o.ext_len[q] = 1;
    o.marker[q] = v.marker[i]; o.left[q] = sl; o.right[q] = sr;
}

// ---- step 6: DSReflectedSubKmerExtractionFromForward -- key' = key[1:] + extension, extension' = key[0], marker 2 ------------------
__global__ __launch_bounds__(256) void k_ks_reflect(const DynView v, int64_t n, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[n] = n;
    if (i >= n) return;
    const int len = (int)v.key_len[i];
    const Pk4 w = pk_load(v.key, i);
    Pk4 r = pk_shl(w, 1);                                            // (the bits behind the last base are 0: so is base len - 1 now)
    pk_or(r, (len - 1) >> 5, pk_at(v.ext[v.ext_off[i]] >> 62, len - 1));
    pk_store(o.key, i, pk_keep4(r, len));
    o.key_len[i] = (uint8_t)len;
    o.ext[i] = w.w0 & (3ull << 62);
    o.ext_off[i] = i;
    o.ext_len[i] = 1;
    o.marker[i] = 2; o.left[i] = v.left[i]; o.right[i] = v.right[i];
}
// ---- step 8: DSSubKmerToFullKmer -- marker 2: extension + key, marker 1: key + extension; marker 1, no extension -----------------
__global__ __launch_bounds__(256) void k_ks_full(const DynView v, int64_t n, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) o.ext_off[n] = 0;
    if (i >= n) return;
    const int len = (int)v.key_len[i];
    const Pk4 w = pk_load(v.key, i);
    const uint64_t e = v.ext[v.ext_off[i]] >> 62;
    Pk4 r;
    if (v.marker[i] == 2) r = Pk4{(w.w0 >> 2) | (e << 62), (w.w1 >> 2) | (w.w0 << 62), (w.w2 >> 2) | (w.w1 << 62), (w.w3 >> 2) | (w.w2 << 62)};
    else { r = w; pk_or(r, len >> 5, pk_at(e, len)); }
    pk_store(o.key, i, pk_keep4(r, len + 1));
    o.key_len[i] = (uint8_t)(len + 1);
    o.ext_off[i] = 0;
    o.ext_len[i] = 0;
    o.marker[i] = 1; o.left[i] = v.left[i]; o.right[i] = v.right[i];
}

// ---- step 9: DSBinaryFullKmerArrayToString -- rows "KMER,marker|left|right\n" of the records whose key has k bases ----------------
__global__ __launch_bounds__(256) void k_ks_text_sizes(const DynView v, int64_t n, int k, uint64_t *__restrict__ sz, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool kp = (int)v.key_len[i] == k;
    keep[i] = kp ? 1u : 0u;
    sz[i] = kp ? (uint64_t)(k + 4 + pk_int_chars(v.marker[i]) + pk_int_chars(v.left[i]) + pk_int_chars(v.right[i])) : 0ull;
}
// the row offsets of the written rows: n_out + 1 entries
__global__ __launch_bounds__(256) void k_ks_text_offsets(const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank, const uint64_t *__restrict__ toff,
                                                         int64_t n, int64_t *__restrict__ row_off) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) row_off[rank[n]] = (int64_t)toff[n];
    if (i < n && keep[i]) row_off[rank[i]] = (int64_t)toff[i];
}
// the pieces of a row's text behind its k-mer: the attributes and how many characters each takes
struct KsRow { int kl, m, l, r, cm, cl, cr; };
__device__ __forceinline__ KsRow ks_row(const DynView &v, int64_t i) {
    const int m = v.marker[i], l = v.left[i], r = v.right[i];
    return KsRow{(int)v.key_len[i], m, l, r, pk_int_chars(m), pk_int_chars(l), pk_int_chars(r)};
}
__device__ __forceinline__ char ks_row_char(const DynView &v, int64_t i, const KsRow &w, int q) {
    if (q < w.kl) return (char)pk_letter(pk_base_of(v.key + KS_KW * i, q));
    q -= w.kl;
    if (q == 0) return ',';
    if (q < 1 + w.cm) return pk_int_char(w.m, q - 1);
    if (q == 1 + w.cm) return '|';
    if (q < 2 + w.cm + w.cl) return pk_int_char(w.l, q - 2 - w.cm);
    if (q == 2 + w.cm + w.cl) return '|';
    if (q < 3 + w.cm + w.cl + w.cr) return pk_int_char(w.r, q - 3 - w.cm - w.cl);
    return '\n';
}
// one thread per chunk of 8 output bytes, up to lim (the smaller of the text's length and the buffer): one search for the row
// that owns the chunk's first byte, then a walk forward over the rows the chunk touches (rows of no bytes are stepped over); the
// chunk goes out in one 8-byte store where it is whole and aligned
__global__ __launch_bounds__(256) void k_ks_text_fill(const DynView v, int64_t n, const uint64_t *__restrict__ toff, int64_t lim, char *__restrict__ out) {
    const int64_t b0 = 8 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (b0 >= lim) return;
    const int cnt = lim - b0 < 8 ? (int)(lim - b0) : 8;
    int64_t i = pk_find(toff, n, b0), beg = (int64_t)toff[i], end = (int64_t)toff[i + 1];
    KsRow w = ks_row(v, i);
    uint64_t pack = 0;
    for (int j = 0; j < 8; j++) {
        if (j >= cnt) break;
        const int64_t b = b0 + j;
        if (b >= end) {                                               // (b < lim <= toff[n]: a row that owns b exists)
            while (b >= end) { i++; beg = end; end = (int64_t)toff[i + 1]; }
            w = ks_row(v, i);
        }
        pack |= (uint64_t)(uint8_t)ks_row_char(v, i, w, (int)(b - beg)) << (8 * j);
    }
    if (cnt == 8 && ((uintptr_t)(out + b0) & 7) == 0) *reinterpret_cast<uint64_t *>(out + b0) = pack;
    else for (int j = 0; j < cnt; j++) out[b0 + j] = (char)(pack >> (8 * j));
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static bool ks_k_ok(int k) { return k >= 8 && k <= 124 && (k - 1) % 31 != 0; }
static int ks_params(rfx_ctx *ctx, const rfx_ksort_params *p, KsParams *o) {
    if (!p) return RFX_E_ARG;
    if (!ks_k_ok(p->k)) { ctx->last_error = "k-mer sorting: k outside 8..124 or (k - 1) % 31 == 0 (32, 63, 94: the reference's classes are broken there)"; return RFX_E_ARG; }
    if (p->min_error_cov <= 0) { ctx->last_error = "k-mer sorting: min_error_cov <= 0 (the reference's classes without error correction cannot run)"; return RFX_E_ARG; }
    if (!(p->min_repeat_fold >= 1.0) || !std::isfinite(p->min_repeat_fold)) { ctx->last_error = "k-mer sorting: min_repeat_fold < 1"; return RFX_E_ARG; }
    if (p->max_k < 1 || p->max_k + 3 > PK_CLAMP || p->max_cov < 0) { ctx->last_error = "k-mer sorting: max_k or max_cov out of range"; return RFX_E_ARG; }
    *o = KsParams{p->k, p->max_k + 3, p->min_error_cov, p->max_cov, p->min_repeat_fold};
    return RFX_OK;
}
static int ks_bad(rfx_ctx *ctx, uint32_t bad) {
    ctx->last_error = bad & KS_BAD_OFFSETS ? "k-mer sorting: row offsets that run backwards"
                    : bad & KS_BAD_COMMA   ? "k-mer sorting: a row without a comma"
                    : bad & KS_BAD_COUNT   ? "k-mer sorting: a count that is not decimal digits"
                                           : "k-mer sorting: a record whose extension is not one base";
    return RFX_E_ARG;
}

// steps 1-4: text in HBM -> a packed set in the library's own buffers
static int ks_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, const KsParams &prm, DynDev &d) {
    if (n == 0) return dyn_empty(ctx, d);
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "k-mer sorting: 2^31 rows or more"; return RFX_E_LIMIT; }
    DevBuf keep, slot, kbeg, cnt, flags;
    RFX_ALLOC(keep, uint32_t, n); RFX_ALLOC(slot, uint64_t, n + 1);
    RFX_ALLOC(kbeg, int64_t, n); RFX_ALLOC(cnt, int32_t, n);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_ks_bin_sizes, n, d_text, d_row_off, n, prm, keep.as<uint32_t>(), kbeg.as<int64_t>(), cnt.as<int32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, keep.as<uint32_t>(), slot.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, slot.as<uint64_t>() + n, nullptr, nullptr, &f));
    if (f.bad) return ks_bad(ctx, f.bad);
    const int64_t n_out = 2 * (int64_t)f.total[0];
    if (n_out == 0) return dyn_empty(ctx, d);
    RFX_TRY(dyn_alloc(ctx, d, n_out, n_out));
    RFX_LAUNCH_N(k_ks_bin_emit, n, d_text, n, prm, keep.as<uint32_t>(), slot.as<uint64_t>(),
                 kbeg.as<int64_t>(), cnt.as<int32_t>(), n_out, dyn_out(d));
    return RFX_OK;
}

// what an operator asks of its input: every extension one base; one_len: keys all of one length; max_len: the longest key allowed
static int ks_check(rfx_ctx *ctx, const CallFlags &f, bool one_len, int max_len) {
    if (f.bad) return ks_bad(ctx, f.bad);
    if (one_len && f.min_len != f.max_len) { ctx->last_error = "k-mer sorting: keys of more than one length"; return RFX_E_ARG; }
    if (f.min_len < 1 || (int)f.max_len > max_len) { ctx->last_error = "k-mer sorting: a key of 0 bases or too long"; return RFX_E_ARG; }
    return RFX_OK;
}

// one fold over a sorted set
static int ks_fold(rfx_ctx *ctx, bool reflected, const DynDev &in, const KsParams &prm, DynDev &out) {
    const int64_t n = in.n;
    if (n == 0) return dyn_empty(ctx, out);
    DevBuf head, rank, flags;
    RFX_ALLOC(head, uint32_t, n); RFX_ALLOC(rank, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    const DynView v = dyn_view(in);
    RFX_LAUNCH_N(k_ks_heads, n, v, n, head.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, head.as<uint32_t>(), rank.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, rank.as<uint64_t>() + n, nullptr, nullptr, &f));
    RFX_TRY(ks_check(ctx, f, true, 124));
    const int64_t ns = (int64_t)f.total[0];
    RFX_TRY(dyn_alloc(ctx, out, ns, ns));
    if (reflected) RFX_LAUNCH_N(k_ks_fold<true>, n, v, n, head.as<uint32_t>(), rank.as<uint64_t>(), prm, dyn_out(out));
    else RFX_LAUNCH_N(k_ks_fold<false>, n, v, n, head.as<uint32_t>(), rank.as<uint64_t>(), prm, dyn_out(out));
    return RFX_OK;
}

// step 6 (full == false) / step 8 (full == true)
static int ks_map(rfx_ctx *ctx, bool full, const DynDev &in, DynDev &out) {
    const int64_t n = in.n;
    if (n == 0) return dyn_empty(ctx, out);
    DevBuf flags;
    RFX_TRY(call_flags_init(ctx, flags));
    const DynView v = dyn_view(in);
    RFX_LAUNCH_N(k_ks_lengths, n, v, n, flags.as<CallFlags>());
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));
    RFX_TRY(ks_check(ctx, f, !full, full ? 123 : 124));
    RFX_TRY(dyn_alloc(ctx, out, n, full ? 0 : n));
    if (full) RFX_LAUNCH_N(k_ks_full, n, v, n, dyn_out(out));
    else RFX_LAUNCH_N(k_ks_reflect, n, v, n, dyn_out(out));
    return RFX_OK;
}

// steps 1-4 from the counter's arrays -> a packed set in the library's own buffers: what ks_binarize gives for their rows
static bool kc_in_ok(const KcIn &in) {
    return in.n >= 0 && in.n_extra >= 0 && (in.count_bytes == 4 || in.count_bytes == 8) && (in.n == 0 || (in.keys && in.counts)) &&
           (in.n_extra == 0 || in.extra);
}
static int kc_k_ok(rfx_ctx *ctx, int k) {
    if (k % 32 != 0) return RFX_OK;
    ctx->last_error = "k-mer sorting from counts: k is a multiple of 32 (the counter writes no keys of that k)";
    return RFX_E_ARG;
}
static int ks_from_counts(rfx_ctx *ctx, const KcIn &in, const KsParams &prm, DynDev &d) {
    const int64_t n = in.n + in.n_extra;
    if (n == 0) return dyn_empty(ctx, d);
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "k-mer sorting: 2^31 rows or more"; return RFX_E_LIMIT; }
    DevBuf keep, slot, flags;
    RFX_ALLOC(keep, uint32_t, n); RFX_ALLOC(slot, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_kc_keep, n, in, prm, keep.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, keep.as<uint32_t>(), slot.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, slot.as<uint64_t>() + n, nullptr, nullptr, &f));
    if (f.bad) { ctx->last_error = "k-mer sorting from counts: a negative count"; return RFX_E_ARG; }
    const int64_t n_out = 2 * (int64_t)f.total[0];
    if (n_out == 0) return dyn_empty(ctx, d);
    RFX_TRY(dyn_alloc(ctx, d, n_out, n_out));
    RFX_LAUNCH_N(k_kc_emit, 2 * n, in, prm, keep.as<uint32_t>(), slot.as<uint64_t>(), n_out, dyn_out(d));
    return RFX_OK;
}

// steps 5-8 behind either binarizer (a is used up); the set stays in HBM between the operators
static int ks_run_set(rfx_ctx *ctx, DynDev &a, const KsParams &prm, int bubble, DynDev &out) {
    DynDev b;
    if (bubble) {
        DevBuf ps;
        uint32_t lmin = 0;
        RFX_TRY(dyn_sort(ctx, a, 1, b, ps, &lmin));
        RFX_TRY(ks_fold(ctx, false, b, prm, a));
        RFX_TRY(ks_map(ctx, false, a, b));
        RFX_TRY(dyn_sort(ctx, b, 1, a, ps, &lmin));
        RFX_TRY(ks_fold(ctx, true, a, prm, b));
        return ks_map(ctx, true, b, out);
    }
    return ks_map(ctx, true, a, out);
}
// steps 1-8 from text
static int ks_run(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const KsParams &prm, int bubble, DynDev &out) {
    DynDev a;
    RFX_TRY(ks_binarize(ctx, d_text, d_row_off, n_rows, prm, a));
    return ks_run_set(ctx, a, prm, bubble, out);
}

// the text of a set into d_text (filled up to cap); *total = its length, *n_rows = its rows; own: a buffer of the library's
static int ks_to_text(rfx_ctx *ctx, const DynDev &d, int k, char *d_text, int64_t cap, int64_t *total, int64_t *d_row_off, int64_t *n_rows, DevBuf *own) {
    const int64_t n = d.n;
    *total = 0; *n_rows = 0;
    if (n == 0) {
        if (d_row_off) RFX_HIP(hipMemsetAsync(d_row_off, 0, 8, ctx->stream));
        if (own) RFX_HIP(own->alloc(1, ctx->stream));
        return sync_checked(ctx);
    }
    DevBuf sz, toff, keep, rank;
    RFX_ALLOC(sz, uint64_t, n); RFX_ALLOC(toff, uint64_t, n + 1);
    RFX_ALLOC(keep, uint32_t, n); RFX_ALLOC(rank, uint64_t, n + 1);
    const DynView v = dyn_view(d);
    RFX_LAUNCH_N(k_ks_text_sizes, n, v, n, k, sz.as<uint64_t>(), keep.as<uint32_t>());
    RFX_TRY(exclusive_scan_u64(ctx, sz.as<uint64_t>(), toff.as<uint64_t>(), n));
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, keep.as<uint32_t>(), rank.as<uint64_t>(), n));
    uint64_t t = 0, nr = 0;
    RFX_TRY(small_readback(ctx, &t, toff.as<uint64_t>() + n, 8));
    RFX_TRY(small_readback(ctx, &nr, rank.as<uint64_t>() + n, 8));
    *total = (int64_t)t; *n_rows = (int64_t)nr;
    if (own) {
        RFX_HIP(own->alloc((size_t)std::max<int64_t>(*total, 1), ctx->stream));
        d_text = own->as<char>(); cap = *total;
    }
    if (d_row_off) {
        RFX_LAUNCH_N(k_ks_text_offsets, n, keep.as<uint32_t>(), rank.as<uint64_t>(),
                     toff.as<uint64_t>(), n, d_row_off);
    }
    const int64_t lim = std::min<int64_t>(*total, cap);
    if (lim > 0) {
        RFX_LAUNCH_N(k_ks_text_fill, ceil_div(lim, 8), v, n, toff.as<uint64_t>(), lim, d_text);
    }
    return sync_checked(ctx);
}

}  // namespace

// DSSubKmerToFullKmer and the text writer for the reduction stage (rfx_reduce.hip), whose classes of the same names are these
int rfx::ks_set_full_kmers(rfx_ctx *ctx, const DynDev &in, DynDev &out) { return ks_map(ctx, true, in, out); }
int rfx::ks_set_to_text(rfx_ctx *ctx, const DynDev &d, int k, char *d_text, int64_t cap, int64_t *total, int64_t *d_row_off, int64_t *n_rows, DevBuf *own) {
    return ks_to_text(ctx, d, k, d_text, cap, total, d_row_off, n_rows, own);
}
// the records of a set whose key has len bases: keep flags, their exclusive scan (n + 1 entries) and the total (nothing allocated for
// an empty set)
int rfx::ks_select_length(rfx_ctx *ctx, const DynDev &in, int len, DevBuf &keep, DevBuf &rank, int64_t *total) {
    *total = 0;
    if (in.n == 0) return RFX_OK;
    RFX_ALLOC(keep, uint32_t, in.n); RFX_ALLOC(rank, uint64_t, in.n + 1);
    RFX_LAUNCH_N(k_ks_len_keep, in.n, in.key_len.as<uint8_t>(), in.n, len, keep.as<uint32_t>());
    return scan_keep(ctx, keep.as<uint32_t>(), in.n, rank.as<uint64_t>(), total);
}

// set j's records of key_lens[j] bases, set after set, as the sub-k-mer records rfx_dyn_binarize form 0 makes of their text rows
int rfx::ks_kmers_to_records(rfx_ctx *ctx, const DynDev *const *sets, const int *key_lens, int n_sets, DynDev &out, int64_t *kept_per_set) {
    std::vector<DevBuf> keep((size_t)n_sets), rank((size_t)n_sets);
    std::vector<int64_t> kept((size_t)n_sets, 0);
    int64_t n_out = 0;
    for (int j = 0; j < n_sets; j++) {
        RFX_TRY(ks_select_length(ctx, *sets[j], key_lens[j], keep[(size_t)j], rank[(size_t)j], &kept[(size_t)j]));
        n_out += kept[(size_t)j];
        if (kept_per_set) kept_per_set[j] = kept[(size_t)j];
    }
    if (n_out == 0) return dyn_empty(ctx, out);
    RFX_TRY(dyn_alloc(ctx, out, n_out, n_out));
    int64_t base = 0;
    for (int j = 0; j < n_sets; j++) {
        if (kept[(size_t)j] == 0) continue;
        const DynDev &s = *sets[j];
        RFX_LAUNCH_N(k_ks_kmer_emit, s.n, dyn_view(s), s.n, keep[(size_t)j].as<uint32_t>(), rank[(size_t)j].as<uint64_t>(), base, n_out, dyn_out(out));
        base += kept[(size_t)j];
    }
    return RFX_OK;
}
// the sorter's parameter check alone
int rfx::ks_params_check(rfx_ctx *ctx, const rfx_ksort_params *params) {
    KsParams prm;
    RFX_TRY(ks_params(ctx, params, &prm));
    return kc_k_ok(ctx, prm.k);
}
// steps 1-8 from the counter's arrays (the body of rfx_dev_ksort_run_counts), for the driver in rfx_reduce.hip
int rfx::ks_run_counts(rfx_ctx *ctx, const uint64_t *d_keys, const void *d_counts, int count_bytes, int64_t n, const uint64_t *d_extra, int64_t n_extra,
                       const rfx_ksort_params *params, DynDev &out) {
    const KcIn in{d_keys, d_counts, n, count_bytes, d_extra, n_extra};
    if (!kc_in_ok(in)) return RFX_E_ARG;
    KsParams prm;
    RFX_TRY(ks_params(ctx, params, &prm));
    RFX_TRY(kc_k_ok(ctx, prm.k));
    DynDev a;
    RFX_TRY(ks_from_counts(ctx, in, prm, a));
    return ks_run_set(ctx, a, prm, params->bubble, out);
}

extern "C" {

void rfx_ksort_default_params(rfx_ksort_params *p, int k) try {
    if (!p) return;
    p->k = k; p->max_k = 95; p->min_error_cov = 8; p->max_cov = 10000000; p->bubble = 1; p->min_repeat_fold = 1.5;
} RFX_API_CATCH_VOID(nullptr)

int rfx_dev_ksort_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_ksort_params *params,
                           rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text, d_row_off, n_rows)) return RFX_E_ARG;
    KsParams prm;
    RFX_TRY(ks_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(ks_binarize(ctx, d_text, d_row_off, n_rows, prm, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_ksort_fork_filter(rfx_ctx *ctx, int reflected, const rfx_dyn_packed *d_sorted, const rfx_ksort_params *params,
                              rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_sorted) || !dyn_packed_out_ok(d_out) || (reflected != 0 && reflected != 1)) return RFX_E_ARG;
    KsParams prm;
    RFX_TRY(ks_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_sorted, a));
    RFX_TRY(ks_fold(ctx, reflected != 0, a, prm, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_ksort_reflect(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(ks_map(ctx, false, a, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_ksort_full_kmers(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(ks_map(ctx, true, a, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_ksort_to_text(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int k, char *d_text, int64_t cap, int64_t *out_len, int64_t *d_row_off,
                          int64_t *n_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !out_len || !n_out || cap < 0 || (cap > 0 && !d_text) || k < 1 || k > 124) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    int64_t total = 0, rows = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(ks_to_text(ctx, a, k, d_text, cap, &total, d_row_off, &rows, nullptr));
    *out_len = total; *n_out = rows;
    return total > cap ? RFX_E_CAP : RFX_OK;
} RFX_API_CATCH(ctx)

int rfx_dev_ksort_run(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_ksort_params *params,
                      rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text, d_row_off, n_rows)) return RFX_E_ARG;
    KsParams prm;
    RFX_TRY(ks_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(ks_run(ctx, d_text, d_row_off, n_rows, prm, params->bubble, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_ksort_from_counts(rfx_ctx *ctx, const uint64_t *d_keys, const void *d_counts, int count_bytes, int64_t n, const uint64_t *d_extra_keys,
                              int64_t n_extra, const rfx_ksort_params *params, rfx_dyn_packed *d_out) try {
    const KcIn in{d_keys, d_counts, n, count_bytes, d_extra_keys, n_extra};
    if (!ctx || !dyn_packed_out_ok(d_out) || !kc_in_ok(in)) return RFX_E_ARG;
    KsParams prm;
    RFX_TRY(ks_params(ctx, params, &prm));
    RFX_TRY(kc_k_ok(ctx, prm.k));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(ks_from_counts(ctx, in, prm, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_ksort_run_counts(rfx_ctx *ctx, const uint64_t *d_keys, const void *d_counts, int count_bytes, int64_t n, const uint64_t *d_extra_keys,
                             int64_t n_extra, const rfx_ksort_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(ks_run_counts(ctx, d_keys, d_counts, count_bytes, n, d_extra_keys, n_extra, params, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_dyn_from_kmers(rfx_ctx *ctx, const rfx_dyn_packed *d_sets, const int *key_lens, int n_sets, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || n_sets < 0 || n_sets > 64 || (n_sets > 0 && (!d_sets || !key_lens))) return RFX_E_ARG;
    for (int j = 0; j < n_sets; j++) {
        if (!dyn_packed_ok(&d_sets[j])) return RFX_E_ARG;
        if (key_lens[j] < 1 || key_lens[j] > 124) { ctx->last_error = "full k-mers to sub-k-mer records: a key length outside 1..124"; return RFX_E_ARG; }
    }
    RFX_HIP(hipSetDevice(ctx->device));
    std::vector<DynDev> in((size_t)n_sets);
    std::vector<const DynDev *> ptr((size_t)n_sets);
    for (int j = 0; j < n_sets; j++) {
        RFX_TRY(dyn_borrow(ctx, &d_sets[j], in[(size_t)j]));
        ptr[(size_t)j] = &in[(size_t)j];
    }
    DynDev a;
    RFX_TRY(ks_kmers_to_records(ctx, ptr.data(), key_lens, n_sets, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

// host text in, host text out; everything between packed and in HBM: upload, run, to-text, one copy back
int rfx_ksort_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, const rfx_ksort_params *params, char *out, int64_t cap,
                   int64_t *out_len) try {
    if (!ctx || !text_rows_ok(text, row_off, n_rows) || !out_len || cap < 0 || (cap > 0 && !out)) return RFX_E_ARG;
    KsParams prm;
    RFX_TRY(ks_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_text, d_off, d_out;
    DynDev a;
    int64_t total = 0, rows = 0;
    RFX_TRY(dyn_upload_text(ctx, text, row_off, n_rows, d_text, d_off));
    RFX_TRY(ks_run(ctx, (const char *)d_text.p, d_off.as<int64_t>(), n_rows, prm, params->bubble, a));
    RFX_TRY(ks_to_text(ctx, a, prm.k, nullptr, 0, &total, nullptr, &rows, &d_out));
    return text_to_host(ctx, {{d_out, total, out, cap, out_len}}, true);
} RFX_API_CATCH(ctx)

}  // extern "C"
