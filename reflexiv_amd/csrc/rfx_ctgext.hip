// rfx_ctgext.hip -- the contig extension stages (Assembly_intermediate/08Extend and 09ExtendAgain) on packed sets that stay in HBM
// (DESIGN.md section 25): P/ReflexivDSDynamicKmerExtend.java, driver `assemblyFromKmer` :125-254, and
// P/ReflexivDSDynamicKmerExtendRoundTwo.java, driver :125-221.
//
// 08Extend runs the ten classes of the contig fixing stage (rfx_fixing.hip); only its first two differ, and only
// they are here: DynamicKmerBinarizerFromReducedToSubKmer (:3118-3219), which reads the rows of 07EndExtend, and
// DSExtractFixingKmerFromContigEnds (:1189-1267), which takes the end 31-mers out of the two consensus ends that 07EndExtend spliced on
// -- left_len windows from the front, right_len from the back -- and cuts the contig back to the original of 05FixingAgain.  Everything
// behind them is rfx::fx_from_ends, the fixing stage's own code.  09ExtendAgain is the second fixing stage's binarizer, loop and contigs
// (rfx_fixing2.hip) behind another header of the text rows, which that file's text writer takes as its third form.
//
// The input is an rfx_endext_set: bases only, the literals "-1l" / "r1-" of a flagged seam in `flags`.  The reference reads every
// character other than A, C and G as T, so a flagged seam is three T bases in the TEXT, at [left_len - 3, left_len) and [T - right_len,
// T - right_len + 3).  One thread per end 31-mer: its contig through the scanned counts, its window out of the words with one or two
// shifts, and where the window meets a seam the window is prefix, one to three T, suffix.  One thread per output word of a long record.
// No thread loops over a contig.
//
// DEVIATIONS from the reference, stated in the header too: a kept contig whose cut part has fewer than 32 characters is RFX_E_ARG for
// the set (the reference turns 31 into an end 31-mer and anything shorter into a record with a short key; 05FixingAgain holds no contig
// below 2 max_k); the distinct 31-mers come out ascending, as in the fixing stage.
#include <algorithm>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

namespace {

#define EX_K 31                      // FixedKmerSize
#define EX_KEY (EX_K - 1)            // the key of every record behind the contig ends
#define EX_LONGEST 303               // characters of a consensus end: 300 bases and the literal of a flagged seam
#define EX_MIN_CUT 32                // the shortest cut contig: a 30-base key and an extension that the folds can tell from a 31-mer's

// what is wrong with a call's input (CallFlags::bad)
enum { EX_BAD_LAYOUT = 1, EX_TOO_LONG = 2, EX_BAD_ID = 4, EX_BAD_SEQ = 8, EX_SHORT_CUT = 16 };

// ---- step 1 from text: the rows ">Contig_<L>_<left>_<right>_<idx>_<ll>_<rl>_<new>,<sequence>" of 07EndExtend ----------------------------
// one thread per row: the seven ints of the ID (fld[k n + i], k = 0..6), where the sequence lies, whether the row is kept (a sequence of
// at least min_len characters, :3157) and the words it takes
__global__ __launch_bounds__(256) void k_ex_rows_parse(const char *__restrict__ text, const int64_t *__restrict__ row_off, int64_t n, int min_len,
                                                       uint32_t *__restrict__ keep, uint32_t *__restrict__ nw, int32_t *__restrict__ fld,
                                                       int64_t *__restrict__ sbeg, int64_t *__restrict__ slen, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = row_off[i];
    int64_t e = row_off[i + 1];
    while (e > b && (text[e - 1] == '\n' || text[e - 1] == '\r')) e--;
    bool ok = e - b >= 8;
#pragma unroll
    for (int j = 0; j < 8; j++) ok = ok && text[b + j] == ">Contig_"[j];
    int64_t p = b + 8;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        int v = 0;
        ok = ok && pk_dec_int(text, p, e, true, true, false, &v) && p < e && text[p] == (k == 6 ? ',' : '_');
        fld[k * n + i] = v;
        p++;
    }
    const int64_t S = ok ? e - p : 0;
    uint32_t bad = ok ? 0u : (uint32_t)EX_BAD_ID;
    if (ok && S > 0 && text[p] == '(') bad |= (uint32_t)EX_BAD_SEQ;
    if (S >= ((int64_t)1 << 30)) bad |= (uint32_t)EX_TOO_LONG;
    if (bad) atomicOr(&flags->bad, bad);
    const bool kept = !bad && S >= min_len;
    keep[i] = kept ? 1u : 0u;
    nw[i] = kept ? (uint32_t)((S + 31) >> 5) : 0u;
    sbeg[i] = p; slen[i] = S;
}
// threads [0, n): a kept row's fields at its rank; threads [n, n + words): one output word each, 32 characters of the sequence, every
// character other than A, C and G as T (the literals of a flagged seam among them)
__global__ __launch_bounds__(256) void k_ex_rows_pack(const char *__restrict__ text, int64_t n, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank,
                                                      const uint64_t *__restrict__ woff, const int32_t *__restrict__ fld, const int64_t *__restrict__ sbeg,
                                                      const int64_t *__restrict__ slen, const EeSetOut o) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t words = (int64_t)woff[n];
    if (t == 0) o.woff[rank[n]] = words;
    if (t < n) {
        if (!keep[t]) return;
        const int64_t q = (int64_t)rank[t];
        o.woff[q] = (int64_t)woff[t];
        o.len[q] = slen[t];
        o.left[q] = fld[1 * n + t]; o.right[q] = fld[2 * n + t]; o.src_idx[q] = fld[3 * n + t];
        o.left_len[q] = fld[4 * n + t]; o.right_len[q] = fld[5 * n + t]; o.new_idx[q] = fld[6 * n + t];
        o.flags[q] = 0;
    } else if (t - n < words) {
        const int64_t w = t - n, i = pk_find(woff, n, w);
        const int64_t b = 32 * (w - (int64_t)woff[i]), m = slen[i] - b;
        const char *s = text + sbeg[i] + b;
        uint64_t x = 0ull;
        for (int j = 0; j < 32; j++) if (j < m) x |= pk_at(pk_code(s[j]), j);
        o.w[w] = x;
    }
}

// ---- step 2: the contig ends ----------------------------------------------------------------------------------------------------------
// a contig as this stage reads it: L bases in the words, T characters in the text (three more per flagged seam), ll / rl characters of
// the two ends, the cut contig [ll, T - rl) of the text = `cut` bases from base ll - 3 fl of the words
struct ExCtg { const uint64_t *w; int L, T, ll, rl, fl, fr, cut; };
__device__ __forceinline__ ExCtg ex_ctg(const EeSetIn &v, int64_t i) {
    ExCtg c;
    const int f = v.flags[i];
    c.w = v.w + v.woff[i];
    c.L = (int)v.len[i]; c.ll = v.left_len[i]; c.rl = v.right_len[i];
    c.fl = f & 1; c.fr = (f >> 1) & 1;
    c.T = c.L + 3 * c.fl + 3 * c.fr;
    c.cut = c.T - c.ll - c.rl;
    return c;
}
// the base that text position x holds (x outside the seams): three fewer behind each flagged seam
__device__ __forceinline__ int ex_base(const ExCtg &c, int x) { return x - (c.fl && x >= c.ll ? 3 : 0) - (c.fr && x >= c.T - c.rl + 3 ? 3 : 0); }

// per contig: its end 31-mers (ll + rl), whether it gives a long record (T >= 2 max_k, :1207) and that record's extension words; the
// layout the header promises is checked here, before anything indexes with it
__global__ __launch_bounds__(256) void k_ex_ends_sizes(const EeSetIn v, int min_len, uint32_t *__restrict__ nk, uint32_t *__restrict__ nl, uint32_t *__restrict__ nw,
                                                       CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n) return;
    const int64_t L = v.len[i];
    const int f = v.flags[i], ll = v.left_len[i], rl = v.right_len[i];
    const int fl = f & 1, fr = (f >> 1) & 1;
    const bool big = L >= ((int64_t)1 << 30);
    const bool bad = L < 0 || v.woff[i + 1] - v.woff[i] != ((L + 31) >> 5) || (i == 0 && v.woff[0] != 0) || (f & ~3) || ll < 3 * fl || ll > EX_LONGEST ||
                     rl < 3 * fr || rl > EX_LONGEST;
    if (bad) atomicOr(&flags->bad, (uint32_t)EX_BAD_LAYOUT);
    if (!bad && big) atomicOr(&flags->bad, (uint32_t)EX_TOO_LONG);
    const int64_t T = L + 3 * fl + 3 * fr, cut = T - ll - rl;
    bool kept = !bad && !big && T >= min_len;
    if (kept && cut < EX_MIN_CUT) { atomicOr(&flags->bad, (uint32_t)EX_SHORT_CUT); kept = false; }
    nk[i] = kept ? (uint32_t)(ll + rl) : 0u;
    nl[i] = kept ? 1u : 0u;
    nw[i] = kept ? (uint32_t)((cut - EX_KEY + 31) >> 5) : 0u;
}
// one thread per 31-mer: item j of contig i = characters [j, j + 31) for j < ll, then [T - i' - 31, T - i') for i' = rl - 1 .. 0
// (:1214-1226); the value holds its first base in bits 61..60.  The cut contig has 32 characters or more, so a window meets one seam
// at most: its characters ahead of the seam, the seam's T bases inside the window, the characters behind it
__global__ __launch_bounds__(256) void k_ex_ends_kmers(const EeSetIn v, const uint64_t *__restrict__ koff, uint64_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)koff[v.n]) return;
    const int64_t i = pk_find(koff, v.n, t);
    const int j = (int)(t - (int64_t)koff[i]);
    const ExCtg c = ex_ctg(v, i);
    const int p = j < c.ll ? j : c.T - EX_K - (c.rl - 1 - (j - c.ll));
    const int s1 = c.ll - 3, s2 = c.T - c.rl;                        // where the seams begin in the text
    const bool on1 = c.fl && p < s1 + 3 && p + EX_K > s1, on2 = c.fr && p < s2 + 3 && p + EX_K > s2;
    uint64_t x = pk_seg32(c.w, c.L, ex_base(c, p));
    if (on1 || on2) {
        const int s = on1 ? s1 : s2;
        const int pre = s > p ? s - p : 0, te = s + 3 - p < EX_K ? s + 3 - p : EX_K;      // the seam covers [pre, te) of the window
        x = pk_keep(x, pre) | (pk_keep(~0ull, te - pre) >> (2 * pre)) | (pk_seg32(c.w, c.L, ex_base(c, s + 3)) >> (2 * te));
    }
    out[t] = x >> 2;
}
// the cut contigs, cut key 30 / rest, left and right kept (:1229-1261): threads [0, 4 m) write the key words and the record's fields,
// threads [4 m, 4 m + words) one extension word each
__global__ __launch_bounds__(256) void k_ex_ends_long(const EeSetIn v, const uint64_t *__restrict__ loff, const uint64_t *__restrict__ woff, const DynOut o) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n = v.n;
    const int64_t m = (int64_t)loff[n], words = (int64_t)woff[n];
    if (t == 0) o.ext_off[m] = words;
    if (t < PK_KW * m) {
        const int64_t q = t / PK_KW, i = pk_find(loff, n, q);
        const int j = (int)(t % PK_KW);
        const ExCtg c = ex_ctg(v, i);
        o.key[t] = j == 0 ? pk_keep(pk_seg32(c.w, c.L, c.ll - 3 * c.fl), EX_KEY) : 0ull;
        if (j == 0) {
            o.key_len[q] = (uint8_t)EX_KEY;
            o.ext_off[q] = (int64_t)woff[i];
            o.ext_len[q] = c.cut - EX_KEY;
            o.marker[q] = 1; o.left[q] = pk_clamp(v.left[i]); o.right[q] = pk_clamp(v.right[i]);
        }
    } else if (t - PK_KW * m < words) {
        const int64_t w = t - PK_KW * m, i = pk_find(woff, n, w);
        const int r = 32 * (int)(w - (int64_t)woff[i]);
        const ExCtg c = ex_ctg(v, i);
        o.ext[w] = pk_keep(pk_seg32(c.w, c.L, c.ll - 3 * c.fl + EX_KEY + r), c.cut - EX_KEY - r);
    }
}

static int ex_bad(rfx_ctx *ctx, uint32_t bad) {
    if (bad & EX_BAD_ID) { ctx->last_error = "contig extension: a row that is not >Contig_ and seven decimal ints, a comma and the sequence"; return RFX_E_ARG; }
    if (bad & EX_BAD_SEQ) { ctx->last_error = "contig extension: a sequence that starts with '('"; return RFX_E_ARG; }
    if (bad & EX_BAD_LAYOUT) { ctx->last_error = "contig extension: a set whose word_off and len disagree, flags outside 0..3, or end lengths that no consensus has"; return RFX_E_ARG; }
    if (bad & EX_TOO_LONG) { ctx->last_error = "contig extension: a contig of 2^30 bases or more"; return RFX_E_LIMIT; }
    if (bad & EX_SHORT_CUT) { ctx->last_error = "contig extension: a contig whose cut part has fewer than 32 characters"; return RFX_E_ARG; }
    return RFX_OK;
}

}  // namespace

// step 1 from text, first half: which rows are kept and what they take
int rfx::ex_rows_plan(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, int max_k, ExRowsPlan &plan) {
    plan.n = n; plan.m = 0; plan.words = 0;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "contig extension: 2^31 rows or more"; return RFX_E_LIMIT; }
    if (n == 0) return RFX_OK;
    DevBuf nw, flags;
    RFX_ALLOC(plan.keep, uint32_t, n); RFX_ALLOC(nw, uint32_t, n); RFX_ALLOC(plan.rank, uint64_t, n + 1); RFX_ALLOC(plan.woff, uint64_t, n + 1);
    RFX_ALLOC(plan.fld, int32_t, 7 * n); RFX_ALLOC(plan.sbeg, int64_t, n); RFX_ALLOC(plan.slen, int64_t, n);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_ex_rows_parse, n, d_text, d_row_off, n, 2 * max_k, plan.keep.as<uint32_t>(), nw.as<uint32_t>(), plan.fld.as<int32_t>(),
                 plan.sbeg.as<int64_t>(), plan.slen.as<int64_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, plan.keep.as<uint32_t>(), nw.as<uint32_t>(), plan.rank.as<uint64_t>(), plan.woff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, plan.rank.as<uint64_t>() + n, plan.woff.as<uint64_t>() + n, nullptr, &f));
    RFX_TRY(ex_bad(ctx, f.bad));
    plan.m = (int64_t)f.total[0]; plan.words = (int64_t)f.total[1];
    return RFX_OK;
}
// second half: the kept rows into arrays that hold plan.m contigs (word_off: plan.m + 1) and plan.words words
int rfx::ex_rows_fill(rfx_ctx *ctx, const char *d_text, const ExRowsPlan &plan, const EeSetOut &o) {
    if (plan.n == 0 || plan.m == 0) {
        RFX_HIP(hipMemsetAsync(o.woff, 0, 8, ctx->stream));
        return RFX_OK;
    }
    RFX_LAUNCH_N(k_ex_rows_pack, plan.n + plan.words, d_text, plan.n, plan.keep.as<uint32_t>(), plan.rank.as<uint64_t>(), plan.woff.as<uint64_t>(),
                 plan.fld.as<int32_t>(), plan.sbeg.as<int64_t>(), plan.slen.as<int64_t>(), o);
    return RFX_OK;
}

// step 2: the long records, and the 31-mers in emission order (contig by contig, the left end's windows and then the right end's)
int rfx::ex_contig_ends(rfx_ctx *ctx, const EeSetIn &s, int max_k, DynDev &out, DevBuf &kmers, int64_t *n_kmers) {
    const int64_t n = s.n;
    *n_kmers = 0;
    RFX_HIP(kmers.alloc(8, ctx->stream));
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "contig extension: 2^31 contigs or more"; return RFX_E_LIMIT; }
    if (n == 0) return dyn_empty(ctx, out);
    DevBuf nk, nl, nw, koff, loff, woff, flags;
    RFX_ALLOC(nk, uint32_t, n); RFX_ALLOC(nl, uint32_t, n); RFX_ALLOC(nw, uint32_t, n);
    RFX_ALLOC(koff, uint64_t, n + 1); RFX_ALLOC(loff, uint64_t, n + 1); RFX_ALLOC(woff, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_ex_ends_sizes, n, s, 2 * max_k, nk.as<uint32_t>(), nl.as<uint32_t>(), nw.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, nk.as<uint32_t>(), nl.as<uint32_t>(), koff.as<uint64_t>(), loff.as<uint64_t>(), n));
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, nw.as<uint32_t>(), woff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, koff.as<uint64_t>() + n, loff.as<uint64_t>() + n, woff.as<uint64_t>() + n, &f));
    RFX_TRY(ex_bad(ctx, f.bad));
    const int64_t n31 = (int64_t)f.total[0], m = (int64_t)f.total[1], words = (int64_t)f.total[2];
    if (n31 >= ((int64_t)1 << 32)) { ctx->last_error = "contig extension: 2^32 end 31-mers or more"; return RFX_E_LIMIT; }
    *n_kmers = n31;
    if (m == 0) return dyn_empty(ctx, out);
    RFX_ALLOC(kmers, uint64_t, std::max<int64_t>(n31, 1));
    RFX_TRY(dyn_alloc(ctx, out, m, words));
    if (n31 > 0) RFX_LAUNCH_N(k_ex_ends_kmers, n31, s, koff.as<uint64_t>(), kmers.as<uint64_t>());
    RFX_LAUNCH_N(k_ex_ends_long, PK_KW * m + words, s, loff.as<uint64_t>(), woff.as<uint64_t>(), dyn_out(out));
    return RFX_OK;
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------
namespace {
const char *const EX_STAGE = "contig extension";
// the rows of 07EndExtend in HBM -> a set in the library's buffers
int ex_set_of_rows(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, int max_k, EeSetDev &s) {
    ExRowsPlan plan;
    RFX_TRY(ex_rows_plan(ctx, d_text, d_row_off, n_rows, max_k, plan));
    RFX_TRY(ee_set_alloc(ctx, s, plan.m, plan.words));
    return ex_rows_fill(ctx, d_text, plan, ee_set_out(s));
}
}  // namespace

extern "C" {

// DynamicKmerBinarizerFromReducedToSubKmer of P/ReflexivDSDynamicKmerExtend.java (:3118-3219), up to the packed set
int rfx_dev_ext_from_text(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_fix_params *params, rfx_endext_set *d_out) try {
    if (!ctx || !text_rows_ok(d_text, d_row_off, n_rows) || !ee_set_ok(d_out)) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, 1, EX_STAGE));
    RFX_HIP(hipSetDevice(ctx->device));
    ExRowsPlan plan;
    RFX_TRY(ex_rows_plan(ctx, d_text, d_row_off, n_rows, params->max_k, plan));
    if (!packed_out_fits(&d_out->set, plan.m, plan.words)) return RFX_E_CAP;
    RFX_TRY(ex_rows_fill(ctx, d_text, plan, ee_set_out(d_out)));
    d_out->set.n = plan.m;
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

// DSExtractFixingKmerFromContigEnds (:1189-1267) + DSgetFixingLongKmer (:514-535) + DSgetFixingKmer (:853-870)
int rfx_dev_ext_contig_ends(rfx_ctx *ctx, const rfx_endext_set *d_in, const rfx_fix_params *params, rfx_dyn_packed *d_out_long, uint64_t *d_kmers,
                            int64_t cap_kmers, int64_t *n_kmers) try {
    if (!ctx || !ee_set_ok(d_in) || d_in->set.n < 0 || !dyn_packed_out_ok(d_out_long) || !n_kmers || cap_kmers < 0 || (cap_kmers > 0 && !d_kmers)) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, 1, EX_STAGE));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev b;
    DevBuf kmers;
    int64_t n31 = 0;
    RFX_TRY(ex_contig_ends(ctx, ee_set_in(d_in), params->max_k, b, kmers, &n31));
    return fx_ends_store(ctx, b, kmers, n31, d_out_long, d_kmers, cap_kmers, n_kmers);
} RFX_API_CATCH(ctx)

// the driver of 08Extend (:125-254) behind its binarizer, the set resident between the operators
int rfx_dev_ext_run(rfx_ctx *ctx, const rfx_endext_set *d_in, int P, const rfx_fix_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !ee_set_ok(d_in) || d_in->set.n < 0 || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, P, EX_STAGE));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev lng, out;
    DevBuf kmers;
    int64_t n31 = 0;
    RFX_TRY(ex_contig_ends(ctx, ee_set_in(d_in), params->max_k, lng, kmers, &n31));
    RFX_TRY(fx_from_ends(ctx, kmers.as<uint64_t>(), n31, lng, P, params->scramble, params->max_iteration, out));
    return dyn_store(ctx, out, d_out);
} RFX_API_CATCH(ctx)

// host form of the driver of 08Extend (:125-254): the text of 07EndExtend in, the text of 08Extend out; everything between packed and in
// HBM: one upload, the set, the contig ends, the fixing stage's steps 4-9, the text, one copy back
int rfx_ext_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                 int64_t *out_len) try {
    if (!ctx || !text_rows_ok(text, row_off, n_rows) || !text_out_ok(out, cap, out_len)) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, P, EX_STAGE));
    if (n_rows >= ((int64_t)1 << 31)) { ctx->last_error = "contig extension: 2^31 rows or more"; return RFX_E_LIMIT; }      // (before a byte is uploaded)
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_text, d_off, kmers, d_o;
    EeSetDev set;
    DynDev lng, a;
    int64_t n31 = 0, total = 0;
    RFX_TRY(dyn_upload_text(ctx, text, row_off, n_rows, d_text, d_off));
    RFX_TRY(ex_set_of_rows(ctx, (const char *)d_text.p, d_off.as<int64_t>(), n_rows, params->max_k, set));
    RFX_TRY(ex_contig_ends(ctx, ee_set_in(set), params->max_k, lng, kmers, &n31));
    RFX_TRY(fx_from_ends(ctx, kmers.as<uint64_t>(), n31, lng, P, params->scramble, params->max_iteration, a));
    RFX_TRY(dyn_to_text(ctx, a, nullptr, 0, &total, &d_o));
    return text_to_host(ctx, {{d_o, total, out, cap, out_len}}, false);
} RFX_API_CATCH(ctx)

// zipWithIndex + TagRowContigRDDID of P/ReflexivDSDynamicKmerExtendRoundTwo.java (:674-692): the rows of 09ExtendAgain
int rfx_dev_ext2_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, char *d_text, int64_t cap, int64_t *out_len) try {
    return fx2_text_call(ctx, 2, d_in, nullptr, nullptr, d_text, cap, out_len);
} RFX_API_CATCH(ctx)

// host form of the driver of 09ExtendAgain (:125-221): the text of 08Extend in, the text of 09ExtendAgain out; one upload, the second
// fixing stage's binarizer, loop and contigs (DSBinaryFixingKmerToFullKmer :415-456), the text (ends 2 reads neither left nor right),
// one copy back
int rfx_ext2_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                  int64_t *out_len) try {
    if (!ctx || !text_rows_ok(text, row_off, n_rows) || !text_out_ok(out, cap, out_len)) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, P, "contig extension, round two"));
    if (n_rows >= ((int64_t)1 << 31)) { ctx->last_error = "contig extension, round two: 2^31 rows or more"; return RFX_E_LIMIT; }      // (before an offset is read)
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_rows;
    CtgDev c;
    int64_t total = 0;
    RFX_TRY(fx2_contigs_of_text(ctx, text, row_off, n_rows, P, params, c));
    RFX_TRY(fx2_text(ctx, fx2_view(c), 2, nullptr, 0, &total, &d_rows));
    return text_to_host(ctx, {{d_rows, total, out, cap, out_len}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"
