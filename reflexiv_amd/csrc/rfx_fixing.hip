// rfx_fixing.hip -- the contig fixing stage (Assembly_intermediate/04Fixing) on packed record sets that stay in HBM (DESIGN.md
// section 19): P/ReflexivDSDynamicKmerFixing.java, driver `assemblyFromKmer` :125-260 --
// DynamicKmerBinarizerFromReducedToSubKmer (:3106-3203), DSExtractFixingKmerFromContigEnds (:1190-1256), DSgetFixingLongKmer
// (:520-541), DSgetFixingKmer (:857-874), groupBy("kmer").count() (:206), DSFixingKmerLeftAndRightMarkerAssignment (:1857-1878),
// union (:213), sort("k-1"), DSFilterForkSubKmerWithErrorCorrection (:2057-2116), DSChangingFixingKmerToReflectedKmer
// (:1571-1608), sort("k-1"), DSFilterForkReflectedSubKmerWithErrorCorrection (:2232-2283), DSExtendFixingKmerLoop (:2371-3104)
// once on the fold's partitions and then behind a sort min(maximumIteration + 1, 17) times (:229-243), and
// DSBinaryFixingKmerWithLongExtensionToString (:262-299).
//
// The record sets are rfx_dyn_packed (rfx_dynamic.hip): four key words per record, 32 bases per word, the first base in the two
// highest bits, every bit past the last base 0 and every unused key word 0 -- every producer here writes those zeros.  From the
// contig ends on every key has FixedKmerSize - 1 = 30 bases in ONE word, which is also the one signed long the reference sorts by.
// The sorts are rfx_dynamic.hip's (dyn_sort), and so are the binarizer (form 1), the loop and the text writer (dyn_binarize,
// dyn_pass, dyn_to_text, all unchanged): with every key 30 bases long the loop is the dynamic-k pass with no prefix relation,
// `extra` = 0 and the stage branches out of reach, which tests/golden/fixing_vectors.npz decides stage by stage.
//
// New here is the work on whole contigs, thousands of bases long and skewed in length, so no thread loops over one.  The contig
// ends: a scan of per-contig output counts, then one thread per 31-mer (a funnel shift out of key||extension or extension||key)
// and one thread per output WORD of a trimmed contig, its record found through the scanned word offsets.  The distinct 31-mers:
// the 62-bit values through the radix sort, head flags, a scan, and the heads straight into one-base records.  The two folds
// have a closed form per run of equal keys inside a partition -- a run with a row longer than one base keeps exactly those rows,
// in order; any other run keeps its LAST row of the smallest base code -- so they are flags, one 64-bit atomicMin per row of a
// run of two or more, and a compaction; no walk.  The reflection re-cuts the same concatenation, one thread per output word.
//
// DEVIATIONS from the reference, stated in the header too: a row whose sub-k-mer exceeds 124 bases is RFX_E_LIMIT for the set
// (the reference would carry it); a ')' behind the extension is dropped as rfx_dyn_binarize form 1 drops it (the reference
// reads it as a base); the distinct 31-mers come out in ascending order where Spark's groupBy gives its hash order (nothing
// from the first fold on depends on it: the vector generator runs every case under two orders).
#include <algorithm>
#include <string>
#include <vector>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

namespace {

#define FX_K 31                      // FixedKmerSize
#define FX_KEY (FX_K - 1)            // the key of every record behind the contig ends

// what is wrong with a call's input (CallFlags::bad)
enum { FX_BAD_KEY = 1, FX_BAD_EXT = 2, FX_BAD_VALUE = 4, FX_TOO_LONG = 8, FX_BAD_OFFSETS = 16 };

// ---- a compaction: output record q := input record idx[q] -------------------------------------------------------------------------------
// AS_ROW (rfx_dev_fix_run_packed): the record as form 1 of the binarizer reads it out of the row k_dyn_text_fill prints of it -- the key's
// and the extension's bases and nothing behind them, the marker through its decimal text, left / right through theirs and clamped
template <bool AS_ROW>
__global__ __launch_bounds__(256) void k_fx_gather_rec(const DynView v, const int64_t *__restrict__ idx, int64_t m, const DynOut o, uint32_t *__restrict__ ew) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    const int64_t i = idx[q];
    if (AS_ROW) {
        pk_store(o.key, q, pk_keep4(pk_load(v.key, i), (int)v.key_len[i]));
        o.marker[q] = pk_int_as_text(v.marker[i]); o.left[q] = pk_clamp(pk_int_as_text(v.left[i])); o.right[q] = pk_clamp(pk_int_as_text(v.right[i]));
    } else {
        const uint64_t *s = v.key + PK_KW * i;
        uint64_t *d = o.key + PK_KW * q;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
        o.marker[q] = v.marker[i]; o.left[q] = v.left[i]; o.right[q] = v.right[i];
    }
    o.key_len[q] = v.key_len[i];
    o.ext_len[q] = v.ext_len[i];
    ew[q] = (uint32_t)((v.ext_len[i] + 31) >> 5);
}
// one thread per output extension word (the grid covers a bound; the exact count is ooff[m])
template <bool AS_ROW>
__global__ __launch_bounds__(256) void k_fx_gather_ext(const DynView v, const int64_t *__restrict__ idx, int64_t m, const uint64_t *__restrict__ ooff,
                                                       uint64_t *__restrict__ oext) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m <= 0 || w >= (int64_t)ooff[m]) return;
    const int64_t q = pk_find(ooff, m, w);
    const int64_t i = idx[q], r = w - (int64_t)ooff[q];
    const uint64_t x = v.ext[v.ext_off[i] + r];
    oext[w] = AS_ROW ? pk_keep(x, v.ext_len[i] - (int)(32 * r)) : x;
}

// ---- step 1: the length filter behind the binarizer ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fx_long_enough(const uint8_t *__restrict__ key_len, const int32_t *__restrict__ ext_len, int64_t n, int min_len,
                                                        uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keep[i] = (int64_t)key_len[i] + ext_len[i] >= min_len ? 1u : 0u;
}
// ... and on a caller's set, which no binarizer made: a key of more than 124 bases, a record without an extension (it has no form-1
// row) and extension offsets that do not follow the lengths (the gather would index with them) are noted, and such a record is not kept
__global__ __launch_bounds__(256) void k_fx_row_long_enough(const DynView v, int64_t n, int min_len, uint32_t *__restrict__ keep, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int kl = (int)v.key_len[i], el = v.ext_len[i];
    const int64_t b = v.ext_off[i], e = v.ext_off[i + 1];
    uint32_t bad = (kl > 124 ? (uint32_t)FX_TOO_LONG : 0u) | (el < 1 ? (uint32_t)FX_BAD_EXT : 0u);
    if (b < 0 || (el >= 1 && e - b != (((int64_t)el + 31) >> 5))) bad |= FX_BAD_OFFSETS;
    if (bad) atomicOr(&flags->bad, bad);
    keep[i] = (!bad && (int64_t)kl + el >= min_len) ? 1u : 0u;
}

// ---- steps 2-3: the contig ends -----------------------------------------------------------------------------------------------------------
// per contig: its 31-mers (0 or 2 (max_k - 30)), whether it gives a long record, and that record's extension words
__global__ __launch_bounds__(256) void k_fx_ends_sizes(const uint8_t *__restrict__ key_len, const int32_t *__restrict__ ext_len, int64_t n, int max_k,
                                                       uint32_t *__restrict__ nk, uint32_t *__restrict__ nl, uint32_t *__restrict__ nw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t L = (int64_t)key_len[i] + ext_len[i];
    const bool ok = L >= 2 * max_k;
    const int cut = max_k - FX_KEY;
    nk[i] = ok ? (uint32_t)(2 * cut) : 0u;
    nl[i] = ok ? 1u : 0u;
    nw[i] = ok ? (uint32_t)((L - 2 * cut - FX_KEY + 31) >> 5) : 0u;
}
// one thread per 31-mer: item 2 j of contig i = bases [j, j + 31), item 2 j + 1 = bases [L - j - 31, L - j); the value holds its
// first base in bits 61..60
__global__ __launch_bounds__(256) void k_fx_ends_kmers(const DynView v, int64_t n, const uint64_t *__restrict__ koff, uint64_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)koff[n]) return;
    const int64_t i = pk_find(koff, n, t);
    const int j = (int)(t - (int64_t)koff[i]);
    const FxCat c = fx_contig(v, i);
    const int L = c.l0 + c.l1;
    out[t] = fx_cat32(c, (j & 1) ? L - (j >> 1) - FX_K : (j >> 1)) >> 2;
}
// the trimmed contigs, bases [cut, L - cut) cut key 30 / rest: threads [0, 4 m) write the key words and the record's fields,
// threads [4 m, 4 m + words) one extension word each
__global__ __launch_bounds__(256) void k_fx_ends_long(const DynView v, int64_t n, int max_k, const uint64_t *__restrict__ loff, const uint64_t *__restrict__ woff,
                                                      const DynOut o) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = (int64_t)loff[n], words = (int64_t)woff[n];
    const int cut = max_k - FX_KEY;
    if (t == 0) o.ext_off[m] = words;
    if (t < PK_KW * m) {
        const int64_t q = t / PK_KW, i = pk_find(loff, n, q);
        const int j = (int)(t % PK_KW);
        const FxCat c = fx_contig(v, i);
        o.key[t] = j == 0 ? pk_keep(fx_cat32(c, cut), FX_KEY) : 0ull;
        if (j == 0) {
            const int l = v.left[i], r = v.right[i];
            o.key_len[q] = (uint8_t)FX_KEY;
            o.ext_off[q] = (int64_t)woff[i];
            o.ext_len[q] = c.l0 + c.l1 - 2 * cut - FX_KEY;
            o.marker[q] = 1; o.left[q] = l > 0 ? max_k + 3 : l; o.right[q] = r > 0 ? max_k + 3 : r;
        }
    } else if (t - PK_KW * m < words) {
        const int64_t w = t - PK_KW * m, i = pk_find(woff, n, w);
        const int64_t r = w - (int64_t)woff[i];
        const FxCat c = fx_contig(v, i);
        const int el = c.l0 + c.l1 - 2 * cut - FX_KEY;
        o.ext[w] = pk_keep(fx_cat32(c, cut + FX_KEY + (int)(32 * r)), el - (int)(32 * r));
    }
}

// ---- steps 4-5: the distinct 31-mers as records, then the long records -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fx_iota(int64_t n, uint32_t *__restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}
// (a value of 2^62 or more is no 31-mer: the sort orders 62 bits only, so it is refused, not compared)
__global__ __launch_bounds__(256) void k_fx_value_heads(const uint64_t *__restrict__ val, int64_t n, uint32_t *__restrict__ head, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || val[i] != val[i - 1]) ? 1u : 0u;
    if (val[i] >> (2 * FX_K)) atomicOr(&flags->bad, (uint32_t)FX_BAD_VALUE);
}
// a head writes record rank[i]: key = the first 30 bases, extension = the last base, attribute (1, -1, -1)
__global__ __launch_bounds__(256) void k_fx_set_kmers(const uint64_t *__restrict__ val, const uint32_t *__restrict__ head, const uint64_t *__restrict__ rank,
                                                      int64_t n, const DynOut o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    const int64_t q = (int64_t)rank[i];
    const uint64_t x = val[i] << 2;
    uint64_t *d = o.key + PK_KW * q;
    d[0] = pk_keep(x, FX_KEY); d[1] = 0; d[2] = 0; d[3] = 0;
    o.key_len[q] = (uint8_t)FX_KEY;
    o.ext[q] = (x << (2 * FX_KEY)) & (3ull << 62);
    o.ext_off[q] = q;
    o.ext_len[q] = 1;
    o.marker[q] = 1; o.left[q] = -1; o.right[q] = -1;
}
// the long records behind the d one-base records: record base + i, its words moved by base (a one-base record takes one word)
__global__ __launch_bounds__(256) void k_fx_set_long(const DynView v, int64_t n, int64_t words, int64_t base, const DynOut o) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) o.ext_off[base + n] = base + words;
    if (t < n) {
        const uint64_t *s = v.key + PK_KW * t;
        uint64_t *d = o.key + PK_KW * (base + t);
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
        o.key_len[base + t] = v.key_len[t];
        o.ext_off[base + t] = base + v.ext_off[t];
        o.ext_len[base + t] = v.ext_len[t];
        o.marker[base + t] = v.marker[t]; o.left[base + t] = v.left[t]; o.right[base + t] = v.right[t];
    }
    if (t < words) o.ext[base + t] = v.ext[t];
}

// ---- what the folds and the reflection ask of their input: keys of 30 bases, extensions of one base or more -------------------------------
__global__ __launch_bounds__(256) void k_fx_check(const DynView v, int64_t n, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t bad = ((int)v.key_len[i] != FX_KEY ? (uint32_t)FX_BAD_KEY : 0u) | (v.ext_len[i] < 1 ? (uint32_t)FX_BAD_EXT : 0u);
    if (bad) atomicOr(&flags->bad, bad);
}

// ---- steps 6 and 8: the two folds ---------------------------------------------------------------------------------------------------------
// the first row of every partition that has rows (head is zeroed before)
__global__ void k_fx_part_heads(const int64_t *__restrict__ ps, int P, uint32_t *__restrict__ head) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p < P && ps[p] < ps[p + 1]) atomicOr(head + ps[p], 1u);
}
__global__ __launch_bounds__(256) void k_fx_key_heads(const uint64_t *__restrict__ key, int64_t n, uint32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || key[PK_KW * i] != key[PK_KW * (i - 1)]) head[i] = 1u;      // (a partition's first row holds 1 already)
}
// a row's word in its run's contest: 0 for a row longer than one base, else the base code and then the row's index counted down --
// the smallest one is the LAST row of the smallest code.  Runs of one row are settled here.
__device__ __forceinline__ uint64_t fx_fold_word(const DynView &v, int64_t i) {
    if (v.ext_len[i] > 1) return 0ull;
    return (1ull << 40) | ((v.ext[v.ext_off[i]] >> 62) << 32) | (uint64_t)(uint32_t)~(uint32_t)i;
}
__global__ __launch_bounds__(256) void k_fx_fold_contest(const DynView v, int64_t n, const uint32_t *__restrict__ head, const uint64_t *__restrict__ run,
                                                         unsigned long long *__restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (head[i] && (i + 1 == n || head[i + 1])) return;            // a run of one
    atomicMin(best + (run[i + 1] - 1), (unsigned long long)fx_fold_word(v, i));
}
__global__ __launch_bounds__(256) void k_fx_fold_keep(const DynView v, int64_t n, const uint32_t *__restrict__ head, const uint64_t *__restrict__ run,
                                                      const unsigned long long *__restrict__ best, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t kp = 1u;
    if (!(head[i] && (i + 1 == n || head[i + 1]))) {
        const uint64_t w = fx_fold_word(v, i);
        kp = (w == 0ull || best[run[i + 1] - 1] == w) ? 1u : 0u;
    }
    keep[i] = kp;
}

// ---- step 7: DSChangingFixingKmerToReflectedKmer -- key = the LAST 30 bases of the contig, extension = its front, marker 2.  The key
// has 30 bases before and after, so every extension keeps its length and its words: threads [0, 4 n) write the key words and the
// fields, threads [4 n, 4 n + words) one extension word each
__global__ __launch_bounds__(256) void k_fx_reflect(const DynView v, int64_t n, const DynOut o) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t words = v.ext_off[n];
    if (t == 0) o.ext_off[n] = words;
    if (t < PK_KW * n) {
        const int64_t i = t / PK_KW;
        const int j = (int)(t % PK_KW);
        const FxCat c = fx_contig(v, i);
        o.key[t] = j == 0 ? pk_keep(fx_cat32(c, c.l0 + c.l1 - FX_KEY), FX_KEY) : 0ull;
        if (j == 0) {
            o.key_len[i] = (uint8_t)FX_KEY;
            o.ext_off[i] = v.ext_off[i];
            o.ext_len[i] = v.ext_len[i];
            o.marker[i] = 2; o.left[i] = v.left[i]; o.right[i] = v.right[i];
        }
    } else if (t - PK_KW * n < words) {
        const int64_t w = t - PK_KW * n, i = pk_find(v.ext_off, n, w);
        const int64_t r = w - v.ext_off[i];
        o.ext[w] = pk_keep(fx_cat32(fx_contig(v, i), (int)(32 * r)), v.ext_len[i] - (int)(32 * r));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
struct FxParams { int max_k, scramble, max_iteration; };

static int fx_params(rfx_ctx *ctx, const rfx_fix_params *p, FxParams *o) {
    if (!p) return RFX_E_ARG;
    if (p->max_k < FX_K || p->max_k > 124) { ctx->last_error = "contig fixing: max_k must be 31..124"; return RFX_E_ARG; }
    if (p->max_iteration < -1) { ctx->last_error = "contig fixing: max_iteration below -1"; return RFX_E_ARG; }
    *o = FxParams{p->max_k, p->scramble, p->max_iteration};
    return RFX_OK;
}
// keys of 30 bases, extensions of one base or more
static int fx_check(rfx_ctx *ctx, const DynDev &in) {
    if (in.n == 0) return RFX_OK;
    DevBuf flags;
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_fx_check, in.n, dyn_view(in), in.n, flags.as<CallFlags>());
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));
    if (f.bad) {
        ctx->last_error = f.bad & FX_BAD_KEY ? "contig fixing: a key that is not 30 bases long" : "contig fixing: a record without an extension";
        return RFX_E_ARG;
    }
    return RFX_OK;
}
// the kept records of a set, in order (keep / rank: n flags and their exclusive scan, rank[n] = m)
template <bool AS_ROW = false>
static int fx_compact(rfx_ctx *ctx, const DynDev &in, const DevBuf &keep, const DevBuf &rank, int64_t m, DynDev &out) {
    if (m == 0) return dyn_empty(ctx, out);
    const int64_t n = in.n;
    DevBuf idx, ew;
    RFX_ALLOC(idx, int64_t, m); RFX_ALLOC(ew, uint32_t, m);
    RFX_TRY(dyn_alloc(ctx, out, m, in.words));
    const DynView v = dyn_view(in);
    RFX_TRY(index_kept(ctx, keep.as<uint32_t>(), rank.as<uint64_t>(), n, idx.as<int64_t>()));
    RFX_LAUNCH_N(k_fx_gather_rec<AS_ROW>, m, v, idx.as<int64_t>(), m, dyn_out(out), ew.as<uint32_t>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, ew.as<uint32_t>(), out.ext_off.as<uint64_t>(), m));
    if (in.words > 0) {
        RFX_LAUNCH_N(k_fx_gather_ext<AS_ROW>, in.words, v, idx.as<int64_t>(), m, out.ext_off.as<uint64_t>(),
                     out.ext.as<uint64_t>());
    }
    return RFX_OK;
}

// step 1: the binarizer (form 1) and its length filter
static int fx_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, const FxParams &prm, DynDev &out) {
    if (n == 0) return dyn_empty(ctx, out);
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "contig fixing: 2^31 rows or more"; return RFX_E_LIMIT; }
    DynDev a;
    RFX_TRY(dyn_binarize(ctx, d_text, d_row_off, n, 1, a));
    DevBuf keep, rank;
    RFX_ALLOC(keep, uint32_t, n); RFX_ALLOC(rank, uint64_t, n + 1);
    RFX_LAUNCH_N(k_fx_long_enough, n, a.key_len.as<uint8_t>(), a.ext_len.as<int32_t>(), n, 2 * prm.max_k,
                 keep.as<uint32_t>());
    int64_t m = 0;
    RFX_TRY(scan_keep(ctx, keep.as<uint32_t>(), n, rank.as<uint64_t>(), &m));
    return fx_compact(ctx, a, keep, rank, m, out);
}

// step 1 on a packed set (a view of the caller's): form 1's reading of every record, then the same filter -- what fx_binarize gives
// for the rows dyn_to_text writes of the set, with no text made
static int fx_binarize_packed(rfx_ctx *ctx, const DynDev &in, const FxParams &prm, DynDev &out) {
    const int64_t n = in.n;
    if (n == 0) return dyn_empty(ctx, out);
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "contig fixing: 2^31 rows or more"; return RFX_E_LIMIT; }
    DevBuf keep, rank, flags;
    RFX_ALLOC(keep, uint32_t, n); RFX_ALLOC(rank, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_fx_row_long_enough, n, dyn_view(in), n, 2 * prm.max_k, keep.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, keep.as<uint32_t>(), rank.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, rank.as<uint64_t>() + n, nullptr, nullptr, &f));
    if (f.bad & FX_TOO_LONG) { ctx->last_error = "dynamic-k: a key longer than 124 bases"; return RFX_E_LIMIT; }
    if (f.bad & FX_BAD_EXT) { ctx->last_error = "contig fixing: a record without an extension has no row"; return RFX_E_ARG; }
    if (f.bad & FX_BAD_OFFSETS) { ctx->last_error = "contig fixing: extension offsets that do not follow the extension lengths"; return RFX_E_ARG; }
    return fx_compact<true>(ctx, in, keep, rank, (int64_t)f.total[0], out);
}

// steps 2-3: the long records, and the 31-mers in emission order (contig by contig, i = 0 .. max_k - 31, left then right)
static int fx_contig_ends(rfx_ctx *ctx, const DynDev &in, const FxParams &prm, DynDev &out, DevBuf &kmers, int64_t *n_kmers) {
    const int64_t n = in.n;
    *n_kmers = 0;
    RFX_HIP(kmers.alloc(8, ctx->stream));
    if (n == 0) return dyn_empty(ctx, out);
    DevBuf nk, nl, nw, koff, loff, woff, flags;
    RFX_ALLOC(nk, uint32_t, n); RFX_ALLOC(nl, uint32_t, n); RFX_ALLOC(nw, uint32_t, n);
    RFX_ALLOC(koff, uint64_t, n + 1); RFX_ALLOC(loff, uint64_t, n + 1);
    RFX_ALLOC(woff, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    const DynView v = dyn_view(in);
    RFX_LAUNCH_N(k_fx_ends_sizes, n, v.key_len, v.ext_len, n, prm.max_k, nk.as<uint32_t>(), nl.as<uint32_t>(), nw.as<uint32_t>());
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, nk.as<uint32_t>(), nl.as<uint32_t>(), koff.as<uint64_t>(), loff.as<uint64_t>(), n));
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, nw.as<uint32_t>(), woff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, koff.as<uint64_t>() + n, loff.as<uint64_t>() + n, woff.as<uint64_t>() + n, &f));
    const int64_t n31 = (int64_t)f.total[0], m = (int64_t)f.total[1], words = (int64_t)f.total[2];
    *n_kmers = n31;
    if (m == 0) return dyn_empty(ctx, out);
    RFX_ALLOC(kmers, uint64_t, n31);
    RFX_TRY(dyn_alloc(ctx, out, m, words));
    RFX_LAUNCH_N(k_fx_ends_kmers, n31, v, n, koff.as<uint64_t>(), kmers.as<uint64_t>());
    RFX_LAUNCH_N(k_fx_ends_long, PK_KW * m + words, v, n, prm.max_k, loff.as<uint64_t>(), woff.as<uint64_t>(),
                 dyn_out(out));
    return RFX_OK;
}

// steps 4-5 up to the union: the distinct 31-mers as one-base records (ascending), then the long records.  d_kmers is left as it is
static int fx_kmer_set(rfx_ctx *ctx, const uint64_t *d_kmers, int64_t n31, const DynDev &lng, DynDev &out) {
    if (n31 >= ((int64_t)1 << 32)) { ctx->last_error = "contig fixing: 2^32 end 31-mers or more"; return RFX_E_LIMIT; }
    int64_t d = 0;
    DevBuf val, idx, tk, tv, head, rank;
    if (n31 > 0) {
        RFX_ALLOC(val, uint64_t, n31); RFX_ALLOC(idx, uint32_t, n31); RFX_ALLOC(tk, uint64_t, n31);
        RFX_ALLOC(tv, uint32_t, n31); RFX_ALLOC(head, uint32_t, n31); RFX_ALLOC(rank, uint64_t, n31 + 1);
        RFX_HIP(hipMemcpyAsync(val.p, d_kmers, (size_t)n31 * 8, hipMemcpyDeviceToDevice, ctx->stream));
        RFX_LAUNCH_N(k_fx_iota, n31, n31, idx.as<uint32_t>());
        RFX_TRY(sort_pairs(ctx, val.as<uint64_t>(), idx.as<uint32_t>(), n31, 2 * FX_K, tk.as<uint64_t>(), tv.as<uint32_t>()));
        DevBuf flags;
        RFX_TRY(call_flags_init(ctx, flags));
        RFX_LAUNCH_N(k_fx_value_heads, n31, val.as<uint64_t>(), n31, head.as<uint32_t>(), flags.as<CallFlags>());
        RFX_TRY(exclusive_scan_u32_to_u64(ctx, head.as<uint32_t>(), rank.as<uint64_t>(), n31));
        CallFlags f{};
        RFX_TRY(call_flags_read(ctx, flags, rank.as<uint64_t>() + n31, nullptr, nullptr, &f));
        if (f.bad) { ctx->last_error = "contig fixing: a 31-mer value of 2^62 or more"; return RFX_E_ARG; }
        d = (int64_t)f.total[0];
    }
    if (d + lng.n == 0) return dyn_empty(ctx, out);
    RFX_TRY(dyn_alloc(ctx, out, d + lng.n, d + lng.words));
    if (d > 0) {
        RFX_LAUNCH_N(k_fx_set_kmers, n31, val.as<uint64_t>(), head.as<uint32_t>(),
                     rank.as<uint64_t>(), n31, dyn_out(out));
    }
    RFX_LAUNCH_N(k_fx_set_long, std::max(lng.n, lng.words), dyn_view(lng), lng.n, lng.words, d, dyn_out(out));
    return RFX_OK;
}

// steps 6 and 8 over a sorted set cut into P partitions.  The two classes are one text (the base compared is the extension's first,
// which is a one-base extension's only one), so `reflected` selects nothing here
static int fx_fold(rfx_ctx *ctx, const DynDev &in, const int64_t *d_ps, int P, DynDev &out, DevBuf &out_ps) {
    const int64_t n = in.n;
    RFX_TRY(part_starts_alloc(ctx, out_ps, P, false));
    RFX_TRY(check_part_starts(ctx, d_ps, P, n, "contig fixing"));
    if (n == 0) {                                                 // (zeroed here, behind the check's read-back: DESIGN.md section 23)
        RFX_HIP(hipMemsetAsync(out_ps.p, 0, (size_t)(P + 1) * sizeof(int64_t), ctx->stream));
        return dyn_empty(ctx, out);
    }
    if (n >= ((int64_t)1 << 32)) { ctx->last_error = "contig fixing: 2^32 records or more"; return RFX_E_LIMIT; }
    RFX_TRY(fx_check(ctx, in));
    DevBuf head, run, best, keep, rank;
    RFX_ALLOC(head, uint32_t, n); RFX_ALLOC(run, uint64_t, n + 1); RFX_ALLOC(best, unsigned long long, n);
    RFX_ALLOC(keep, uint32_t, n); RFX_ALLOC(rank, uint64_t, n + 1);
    RFX_HIP(hipMemsetAsync(head.p, 0, (size_t)n * 4, ctx->stream));
    RFX_HIP(hipMemsetAsync(best.p, 0xFF, (size_t)n * 8, ctx->stream));
    const DynView v = dyn_view(in);
    RFX_LAUNCH(k_fx_part_heads, dim3(1), dim3(64), 0, d_ps, P, head.as<uint32_t>());
    RFX_LAUNCH_N(k_fx_key_heads, n, v.key, n, head.as<uint32_t>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, head.as<uint32_t>(), run.as<uint64_t>(), n));
    RFX_LAUNCH_N(k_fx_fold_contest, n, v, n, head.as<uint32_t>(), run.as<uint64_t>(),
                 best.as<unsigned long long>());
    RFX_LAUNCH_N(k_fx_fold_keep, n, v, n, head.as<uint32_t>(), run.as<uint64_t>(),
                 best.as<unsigned long long>(), keep.as<uint32_t>());
    int64_t m = 0;
    RFX_TRY(scan_keep(ctx, keep.as<uint32_t>(), n, rank.as<uint64_t>(), &m));
    RFX_TRY(out_part_starts(ctx, d_ps, P, rank.as<uint64_t>(), out_ps.as<int64_t>()));
    return fx_compact(ctx, in, keep, rank, m, out);
}

// step 7
static int fx_reflect(rfx_ctx *ctx, const DynDev &in, DynDev &out) {
    const int64_t n = in.n;
    if (n == 0) return dyn_empty(ctx, out);
    RFX_TRY(fx_check(ctx, in));
    RFX_TRY(dyn_alloc(ctx, out, n, in.words));
    RFX_LAUNCH_N(k_fx_reflect, PK_KW * n + in.words, dyn_view(in), n, dyn_out(out));
    return RFX_OK;
}

// steps 2-3 on step 1's set, then rfx::fx_from_ends
static int fx_run_binarized(rfx_ctx *ctx, const DynDev &a, int P, const FxParams &prm, DynDev &out) {
    DynDev b;
    DevBuf kmers;
    int64_t n31 = 0;
    RFX_TRY(fx_contig_ends(ctx, a, prm, b, kmers, &n31));
    return fx_from_ends(ctx, kmers.as<uint64_t>(), n31, b, P, prm.scramble, prm.max_iteration, out);
}
static int fx_run(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, int P, const FxParams &prm, DynDev &out) {
    DynDev a;
    RFX_TRY(fx_binarize(ctx, d_text, d_row_off, n_rows, prm, a));
    return fx_run_binarized(ctx, a, P, prm, out);
}

}  // namespace

// steps 4-9 behind the contig ends; the set stays in HBM between the operators.  The loop is the dynamic-k pass below iteration 61
// (stage 1): once on the right fold's partitions without a sort, then behind a sort min(max_iteration + 1, 17) times
int rfx::fx_from_ends(rfx_ctx *ctx, const uint64_t *d_kmers, int64_t n31, const DynDev &lng, int P, int scramble, int max_iteration, DynDev &out) {
    DynDev a, b;
    DevBuf ps, ops;
    uint32_t lmin = 0;
    const int start_marker = scramble == 3 ? 1 : 2;
    RFX_TRY(fx_kmer_set(ctx, d_kmers, n31, lng, a));
    RFX_TRY(dyn_sort(ctx, a, P, b, ps, &lmin));
    RFX_TRY(fx_fold(ctx, b, ps.as<int64_t>(), P, a, ops));
    RFX_TRY(fx_reflect(ctx, a, b));
    RFX_TRY(dyn_sort(ctx, b, P, a, ps, &lmin));
    RFX_TRY(fx_fold(ctx, a, ps.as<int64_t>(), P, b, ops));
    RFX_TRY(dyn_pass(ctx, b, ops.as<int64_t>(), P, b.n ? FX_KEY : 0, 1, 5, start_marker, out, nullptr));
    const int rounds = std::min(max_iteration + 1, 17);
    for (int it = 0; it < rounds; it++) {
        DynDev s;
        RFX_TRY(dyn_sort(ctx, out, P, s, ps, &lmin));
        RFX_TRY(dyn_pass(ctx, s, ps.as<int64_t>(), P, lmin, 1, 5, start_marker, out, nullptr));
        RFX_TRY(sync_checked(ctx));                               // (s and the pass's temporaries are read until here)
    }
    return RFX_OK;
}

// ... for the driver from reads to contigs (rfx_meta.hip): the body of rfx_dev_fix_run_packed on a set of the library's (params checked)
int rfx::fx_run_set(rfx_ctx *ctx, const DynDev &in, int P, const rfx_fix_params &params, DynDev &out) {
    const FxParams prm{params.max_k, params.scramble, params.max_iteration};
    DynDev a;
    RFX_TRY(fx_binarize_packed(ctx, in, prm, a));
    return fx_run_binarized(ctx, a, P, prm, out);
}

int rfx::fx_ends_store(rfx_ctx *ctx, const DynDev &lng, const DevBuf &kmers, int64_t n31, rfx_dyn_packed *d_out_long, uint64_t *d_kmers, int64_t cap_kmers,
                       int64_t *n_kmers) {
    *n_kmers = n31;
    if (n31 > cap_kmers || lng.n > d_out_long->cap_n || lng.words > d_out_long->cap_words) {
        d_out_long->n = lng.n; d_out_long->need_words = lng.words;
        return RFX_E_CAP;
    }
    if (n31 > 0) RFX_HIP(hipMemcpyAsync(d_kmers, kmers.p, (size_t)n31 * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return dyn_store(ctx, lng, d_out_long);
}

extern "C" {

void rfx_fix_default_params(rfx_fix_params *p, int max_k) try {
    if (!p) return;
    p->max_k = max_k; p->scramble = 2; p->max_iteration = 150;
} RFX_API_CATCH_VOID(nullptr)

int rfx_dev_fix_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_fix_params *params,
                         rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text, d_row_off, n_rows)) return RFX_E_ARG;
    FxParams prm;
    RFX_TRY(fx_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(fx_binarize(ctx, d_text, d_row_off, n_rows, prm, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_fix_contig_ends(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_fix_params *params, rfx_dyn_packed *d_out_long, uint64_t *d_kmers,
                            int64_t cap_kmers, int64_t *n_kmers) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out_long) || !n_kmers || cap_kmers < 0 || (cap_kmers > 0 && !d_kmers)) return RFX_E_ARG;
    FxParams prm;
    RFX_TRY(fx_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf kmers;
    int64_t n31 = 0;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(fx_contig_ends(ctx, a, prm, b, kmers, &n31));
    return fx_ends_store(ctx, b, kmers, n31, d_out_long, d_kmers, cap_kmers, n_kmers);
} RFX_API_CATCH(ctx)

int rfx_dev_fix_kmer_set(rfx_ctx *ctx, const uint64_t *d_kmers, int64_t n_kmers, const rfx_dyn_packed *d_long, rfx_dyn_packed *d_out) try {
    if (!ctx || n_kmers < 0 || (n_kmers > 0 && !d_kmers) || !dyn_packed_ok(d_long) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_long, a));
    RFX_TRY(fx_check(ctx, a));
    RFX_TRY(fx_kmer_set(ctx, d_kmers, n_kmers, a, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_fix_fork_filter(rfx_ctx *ctx, int reflected, const rfx_dyn_packed *d_sorted, const int64_t *d_part_start, int P, rfx_dyn_packed *d_out,
                            int64_t *d_out_part_start) try {
    if (!ctx || !dyn_packed_ok(d_sorted) || !dyn_packed_out_ok(d_out) || !d_part_start || !d_out_part_start || !parts_ok(P) || (reflected != 0 && reflected != 1))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    DevBuf ops;
    RFX_TRY(dyn_borrow(ctx, d_sorted, a));
    RFX_TRY(fx_fold(ctx, a, d_part_start, P, b, ops));
    RFX_TRY(dyn_store(ctx, b, d_out));                                // (both capacities are checked before anything is copied)
    return part_starts_store(ctx, d_out_part_start, ops, P);
} RFX_API_CATCH(ctx)

int rfx_dev_fix_reflect(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(fx_reflect(ctx, a, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_fix_run(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, int P, const rfx_fix_params *params,
                    rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text, d_row_off, n_rows) || !parts_ok(P)) return RFX_E_ARG;
    FxParams prm;
    RFX_TRY(fx_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(fx_run(ctx, d_text, d_row_off, n_rows, P, prm, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

// the last iteration's set straight into the stage: no text between them
int rfx_dev_fix_run_packed(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, const rfx_fix_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_in) || !dyn_packed_out_ok(d_out) || !parts_ok(P)) return RFX_E_ARG;
    FxParams prm;
    RFX_TRY(fx_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev in, a, o;
    RFX_TRY(dyn_borrow(ctx, d_in, in));
    RFX_TRY(fx_binarize_packed(ctx, in, prm, a));
    RFX_TRY(fx_run_binarized(ctx, a, P, prm, o));
    return dyn_store(ctx, o, d_out);
} RFX_API_CATCH(ctx)

// host text in, host text out; everything between packed and in HBM: upload, run, to-text, one copy back
int rfx_fix_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                 int64_t *out_len) try {
    if (!ctx || !text_rows_ok(text, row_off, n_rows) || !parts_ok(P) || !out_len || cap < 0 || (cap > 0 && !out)) return RFX_E_ARG;
    FxParams prm;
    RFX_TRY(fx_params(ctx, params, &prm));
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_text, d_off, d_o;
    DynDev a;
    int64_t total = 0;
    RFX_TRY(dyn_upload_text(ctx, text, row_off, n_rows, d_text, d_off));
    RFX_TRY(fx_run(ctx, (const char *)d_text.p, d_off.as<int64_t>(), n_rows, P, prm, a));
    RFX_TRY(dyn_to_text(ctx, a, nullptr, 0, &total, &d_o));
    return text_to_host(ctx, {{d_o, total, out, cap, out_len}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"
