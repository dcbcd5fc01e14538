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
// funnel shift); k_ks_heads + a scan + k_ks_fold<REFLECTED> (the thread at a run's head walks the run with the reference's
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
// One thread per row; a kept row writes records 2 s and 2 s + 1 (s = its rank among the kept rows): the k-mer's and then its
// reverse complement's.  key = the first k - 1 bases, extension = base k - 1 at the top of one word, marker 1, left = right =
// the clamped count.
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
    // reverse complement: complement every base, reverse the 128 groups (the k-mer is then the LAST k), move it to the front
    const Pk4 rv{pk_rev2(~f.w3), pk_rev2(~f.w2), pk_rev2(~f.w1), pk_rev2(~f.w0)};
    const Pk4 rc = pk_keep4(pk_shl(rv, 128 - k), k);
    const int32_t c = cnt[r];
    for (int h = 0; h < 2; h++) {
        const Pk4 &w = h ? rc : f;
        const int64_t q = 2 * (int64_t)slot[r] + h;
        pk_store(o.key, q, pk_keep4(w, k - 1));
        o.key_len[q] = (uint8_t)(k - 1);
        o.ext[q] = pk_base(w, k - 1) << 62;
        o.ext_off[q] = q;
        o.ext_len[q] = 1;
        o.marker[q] = 1; o.left[q] = c; o.right[q] = c;
    }
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

// steps 1-8; the set stays in HBM between the operators
static int ks_run(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const KsParams &prm, int bubble, DynDev &out) {
    DynDev a, b;
    RFX_TRY(ks_binarize(ctx, d_text, d_row_off, n_rows, prm, a));
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
