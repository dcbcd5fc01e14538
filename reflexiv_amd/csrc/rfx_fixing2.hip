// rfx_fixing2.hip -- the second contig fixing stage (Assembly_intermediate/05FixingAgain and 06ContigEnds) on packed sets that stay
// in HBM: P/ReflexivDSDynamicKmerFixingRoundTwo.java, driver `assemblyFromKmer` :138-263 --
// DynamicKmerBinarizerFromReducedToSubKmer (:562-752, no length filter), [sort("k-1"), DSExtendFixingKmerLoop] min(maximumIteration
// + 1, 29) times (:203-213), DSBinaryFixingKmerWithLongExtensionToString (:293-560), zipWithIndex + TagStringContigRDDID (:987-1005)
// and DSExtractContigEndsForAlignment (:265-291).
//
// The binarizer (form 1), the sort and the loop are rfx_dynamic.hip's, unchanged (dyn_binarize, dyn_sort, dyn_pass): the loop of
// this file of the reference is the one of the first fixing stage, and tests/golden/fixing2_vectors.npz decides pass by pass that
// with 30-base keys it is the dynamic-k pass.  New here:
//   the contigs      key || extension or extension || key of every record of at least 2 max_k bases as a packed contig set
//                    (rfx_contigs_packed): a keep flag and a word count per record, one scan of both, then ONE THREAD PER OUTPUT
//                    WORD -- 32 bases at offset 32 j of the concatenation, two funnel shifts at most (fx_cat32), masked at the
//                    contig's end.  No thread loops over a contig.
//   the text writer  both files are records of header characters and runs of bases.  Sizes per record (decimal digit counts, the
//                    separators, L or 200 + 200 bases), a scan, then one thread per 16-BYTE CHUNK of the output: one search for the
//                    chunk's first byte, a step to the next record where the chunk crosses a record's end, 16 bases out of one or
//                    two packed words where the chunk lies inside a run of bases, and one 16-byte store.  Chunks are cut at the
//                    16-byte boundaries of the destination ADDRESS, so every whole chunk is an aligned store; the chunk at the
//                    buffer's unaligned head, the one at its tail and the one at `cap` store bytes.
#include <algorithm>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

namespace {

#define FX2_KEY 30                   // FixedKmerSize - 1: the key of every record of 04Fixing
#define FX2_END 200                  // bases of a contig end (:278-279); a contig of 2 FX2_END bases or more gives two ends

// what is wrong with a call's input (CallFlags::bad)
enum { FX2_BAD_KEY = 1, FX2_BAD_EXT = 2, FX2_BAD_LAYOUT = 4, FX2_TOO_LONG = 8, FX2_LINE_BREAK = 16 };

// ---- what the stage asks of its records: keys of 30 bases (ONE long in the reference), extensions of one base or more -----------
__global__ __launch_bounds__(256) void k_fx2_check(const uint8_t *__restrict__ key_len, const int32_t *__restrict__ ext_len, int64_t n,
                                                   CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t bad = ((int)key_len[i] != FX2_KEY ? (uint32_t)FX2_BAD_KEY : 0u) | (ext_len[i] < 1 ? (uint32_t)FX2_BAD_EXT : 0u);
    if (bad) atomicOr(&flags->bad, bad);
}

// ---- step 3: the contigs -----------------------------------------------------------------------------------------------------
// per record: whether its contig is kept (key_len + ext_len >= 2 max_k) and the words it takes
__global__ __launch_bounds__(256) void k_fx2_cat_sizes(const uint8_t *__restrict__ key_len, const int32_t *__restrict__ ext_len, int64_t n, int min_len,
                                                       uint32_t *__restrict__ keep, uint32_t *__restrict__ nw, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t L = (int64_t)key_len[i] + ext_len[i];
    if (ext_len[i] < 0) atomicOr(&flags->bad, (uint32_t)FX2_BAD_EXT);
    if (L >= ((int64_t)1 << 30)) atomicOr(&flags->bad, (uint32_t)FX2_TOO_LONG);
    const bool ok = ext_len[i] >= 0 && L < ((int64_t)1 << 30) && L >= min_len;
    keep[i] = ok ? 1u : 0u;
    nw[i] = ok ? (uint32_t)((L + 31) >> 5) : 0u;
}
// threads [0, n): a kept record writes its contig's fields at its rank; threads [n, n + words): one output word each, its record
// found through the scanned word offsets (a dropped record takes no words and is skipped by the search)
__global__ __launch_bounds__(256) void k_fx2_cat(const DynView v, int64_t n, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank,
                                                 const uint64_t *__restrict__ woff, uint64_t *__restrict__ ow, int64_t *__restrict__ owoff,
                                                 int64_t *__restrict__ olen, int32_t *__restrict__ oleft, int32_t *__restrict__ oright) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t words = (int64_t)woff[n];
    if (t == 0) owoff[rank[n]] = words;
    if (t < n) {
        if (!keep[t]) return;
        const int64_t q = (int64_t)rank[t];
        owoff[q] = (int64_t)woff[t];
        olen[q] = (int64_t)v.key_len[t] + v.ext_len[t];
        oleft[q] = v.left[t]; oright[q] = v.right[t];
    } else if (t - n < words) {
        const int64_t w = t - n, i = pk_find(woff, n, w);
        const int r = (int)(w - (int64_t)woff[i]);
        const FxCat c = fx_contig(v, i);
        ow[w] = pk_keep(fx_cat32(c, 32 * r), c.l0 + c.l1 - 32 * r);
    }
}

// ---- steps 4-5: the two texts ------------------------------------------------------------------------------------------------
// a record of any of the texts: "Contig_<L>_<left>_<right>_<idx>" is its ID of h characters; ends 2 (the rows of 09ExtendAgain,
// TagRowContigRDDID of P/ReflexivDSDynamicKmerExtendRoundTwo.java :674-692): ">Contig-<L>-<idx>", no left / right (never read)
#define FX2_LINE_MAX 10000000        // a contig of that many bases or more is refused for ends 2 (the reference's changeLine would break the field)
struct Fx2Rec { int L, left, right, idx, cL, cl, cr, h; const uint64_t *w; };
__device__ __forceinline__ int fx2_id_chars(int cL, int left, int right, int idx, int ends) {
    return ends == 2 ? 8 + cL + 1 + pk_int_chars(idx) : 7 + cL + 1 + pk_int_chars(left) + 1 + pk_int_chars(right) + 1 + pk_int_chars(idx);
}
__device__ __forceinline__ Fx2Rec fx2_rec(const uint64_t *__restrict__ words, const int64_t *__restrict__ woff, const int64_t *__restrict__ len,
                                          const int32_t *__restrict__ left, const int32_t *__restrict__ right, int64_t i, int ends) {
    Fx2Rec r;
    r.L = (int)len[i]; r.left = ends == 2 ? 0 : left[i]; r.right = ends == 2 ? 0 : right[i]; r.idx = (int)i;
    r.cL = pk_int_chars(r.L); r.cl = pk_int_chars(r.left); r.cr = pk_int_chars(r.right);
    r.h = fx2_id_chars(r.cL, r.left, r.right, r.idx, ends);
    r.w = words + woff[i];
    return r;
}
__device__ __forceinline__ char fx2_id_char(const Fx2Rec &r, int q, int ends) {
    if (ends == 2) {
        if (q < 8) return ">Contig-"[q];
        q -= 8;
        if (q < r.cL) return pk_int_char(r.L, q);
        q -= r.cL;
        return q == 0 ? '-' : pk_int_char(r.idx, q - 1);
    }
    if (q < 7) return "Contig_"[q];
    q -= 7;
    if (q < r.cL) return pk_int_char(r.L, q);
    q -= r.cL;
    if (q == 0) return '_';
    if (q < 1 + r.cl) return pk_int_char(r.left, q - 1);
    q -= 1 + r.cl;
    if (q == 0) return '_';
    if (q < 1 + r.cr) return pk_int_char(r.right, q - 1);
    q -= 1 + r.cr;
    return q == 0 ? '_' : pk_int_char(r.idx, q - 1);
}
// bytes of a record.  ends 0 and 2: "<ID>,<contig>\n".  ends 1: L >= 400 gives ">ID-L\n" + bases [0, 200) + "\n" + ">ID-R\n" + bases
// [L - 200, L) + "\n", anything shorter ">ID\n" + the contig + "\n"
__device__ __forceinline__ int64_t fx2_rec_bytes(int L, int h, int ends) {
    if (ends != 1) return (int64_t)h + 1 + L + 1;
    return L >= 2 * FX2_END ? 2 * ((int64_t)h + 4 + FX2_END + 1) : (int64_t)h + 2 + L + 1;
}
// byte q of a record: a character, or (ch = 0) base *t of the contig with *run bases of that run left, this one included
__device__ __forceinline__ char fx2_byte(const Fx2Rec &r, int ends, int64_t q, int *t, int *run) {
    if (ends != 1) {
        if (q < r.h) return fx2_id_char(r, (int)q, ends);
        if (q == r.h) return ',';
        q -= r.h + 1;
        if (q >= r.L) return '\n';
        *t = (int)q; *run = r.L - (int)q;
        return 0;
    }
    if (q == 0) return '>';
    if (r.L < 2 * FX2_END) {
        if (q < 1 + r.h) return fx2_id_char(r, (int)q - 1, 0);
        q -= 1 + r.h;
        if (q == 0) return '\n';
        q -= 1;
        if (q >= r.L) return '\n';
        *t = (int)q; *run = r.L - (int)q;
        return 0;
    }
    const int half = r.h + 4 + FX2_END + 1;
    const bool right = q >= half;
    if (right) q -= half;
    if (q == 0) return '>';
    if (q < 1 + r.h) return fx2_id_char(r, (int)q - 1, 0);
    q -= 1 + r.h;
    if (q == 0) return '-';
    if (q == 1) return right ? 'R' : 'L';
    if (q == 2) return '\n';
    q -= 3;
    if (q >= FX2_END) return '\n';
    *t = (right ? r.L - FX2_END : 0) + (int)q; *run = FX2_END - (int)q;
    return 0;
}

// per contig: the bytes of its record; the layout the header promises is checked here, before anything indexes with it
__global__ __launch_bounds__(256) void k_fx2_text_sizes(const int64_t *__restrict__ woff, const int64_t *__restrict__ len, const int32_t *__restrict__ left,
                                                        const int32_t *__restrict__ right, int64_t n, int ends, uint64_t *__restrict__ sz,
                                                        CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t L = len[i];
    const bool bad = L < 0 || woff[i + 1] - woff[i] != ((L + 31) >> 5) || (i == 0 && woff[0] != 0);
    if (bad) atomicOr(&flags->bad, (uint32_t)FX2_BAD_LAYOUT);
    if (!bad && L >= ((int64_t)1 << 30)) atomicOr(&flags->bad, (uint32_t)FX2_TOO_LONG);
    if (!bad && ends == 2 && L >= FX2_LINE_MAX) atomicOr(&flags->bad, (uint32_t)FX2_LINE_BREAK);
    const int Lc = bad || L >= ((int64_t)1 << 30) ? 0 : (int)L;
    const int h = fx2_id_chars(pk_int_chars(Lc), ends == 2 ? 0 : left[i], ends == 2 ? 0 : right[i], (int)i, ends);
    sz[i] = (uint64_t)fx2_rec_bytes(Lc, h, ends);
}
// one thread per 16-byte chunk of the destination: chunk c holds the text's bytes [16 c - skew, 16 c - skew + 16) cut to [0, lim),
// skew = the destination address mod 16, so a whole chunk is a 16-byte-aligned store
__global__ __launch_bounds__(256) void k_fx2_text_fill(const uint64_t *__restrict__ words, const int64_t *__restrict__ woff, const int64_t *__restrict__ len,
                                                       const int32_t *__restrict__ left, const int32_t *__restrict__ right, int64_t n, int ends,
                                                       const uint64_t *__restrict__ toff, int64_t lim, int skew, int64_t chunks, char *__restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    const int64_t start = 16 * c - skew;
    const int64_t b0 = start < 0 ? 0 : start, b1 = start + 16 < lim ? start + 16 : lim;
    const bool whole = b1 - b0 == 16;
    int64_t i = pk_find(toff, n, b0);
    Fx2Rec r = fx2_rec(words, woff, len, left, right, i, ends);
    int64_t q = b0 - (int64_t)toff[i], next = (int64_t)toff[i + 1];
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    int t = 0, run = 0;
    const char first = fx2_byte(r, ends, q, &t, &run);
    if (whole && first == 0 && run >= 16) {
        // 16 bases out of one or two words
        const Pk16 y = pk_letters16(r.w, t);
        o[0] = y.a; o[1] = y.b; o[2] = y.c; o[3] = y.d;
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t b = b0 + j;
            if (b < b1) {
                if (b >= next) {                                  // the chunk crosses into the next record
                    i++;
                    r = fx2_rec(words, woff, len, left, right, i, ends);
                    q = 0; next = (int64_t)toff[i + 1];
                }
                char ch = fx2_byte(r, ends, q, &t, &run);
                if (ch == 0) ch = (char)pk_letter(pk_base_of(r.w, t));
                o[j >> 2] |= (uint32_t)(uint8_t)ch << (8 * (j & 3));
                q++;
            }
        }
    }
    if (whole) {
        *reinterpret_cast<uint4 *>(out + b0) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) if (b0 + j < b1) out[b0 + j] = (char)(o[j >> 2] >> (8 * (j & 3)));
    }
}

// keys of 30 bases, extensions of one base or more
static int fx2_check(rfx_ctx *ctx, const DynDev &in) {
    if (in.n == 0) return RFX_OK;
    DevBuf flags;
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_fx2_check, in.n, in.key_len.as<uint8_t>(), in.ext_len.as<int32_t>(), in.n,
                 flags.as<CallFlags>());
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));
    if (f.bad) {
        ctx->last_error = f.bad & FX2_BAD_KEY ? "contig fixing, round two: a key that is not 30 bases long" : "contig fixing, round two: a record without an extension";
        return RFX_E_ARG;
    }
    return RFX_OK;
}

}  // namespace

// step 1: the binarizer (form 1), no length filter; a key that is not 30 bases long or a row without an extension is refused
int rfx::fx2_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, DynDev &out) {
    if (n == 0) return dyn_empty(ctx, out);
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "contig fixing, round two: 2^31 rows or more"; return RFX_E_LIMIT; }
    RFX_TRY(dyn_binarize(ctx, d_text, d_row_off, n, 1, out));
    return fx2_check(ctx, out);
}

// step 2: min(max_iteration + 1, 29) x (sort, loop), the set resident in HBM; zero rounds copy the set.  The loop is the dynamic-k
// pass below iteration 61 (stage 1), as in rfx_fixing.hip
int rfx::fx2_run(rfx_ctx *ctx, const DynDev &in, int P, int scramble, int max_iteration, DynDev &out) {
    if (in.n == 0) return dyn_empty(ctx, out);
    RFX_TRY(fx2_check(ctx, in));
    const int rounds = std::min(max_iteration + 1, 29);
    const int start_marker = scramble == 3 ? 1 : 2;
    if (rounds <= 0) {
        const int64_t n = in.n, words = in.words;
        RFX_TRY(dyn_alloc(ctx, out, n, words));
        auto cp = [&](DevBuf &d, const DevBuf &s, size_t bytes) { return bytes ? hipMemcpyAsync(d.p, s.p, bytes, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess; };
        RFX_HIP(cp(out.key, in.key, (size_t)n * PK_KW * 8)); RFX_HIP(cp(out.key_len, in.key_len, (size_t)n));
        RFX_HIP(cp(out.ext, in.ext, (size_t)words * 8)); RFX_HIP(cp(out.ext_off, in.ext_off, (size_t)(n + 1) * 8));
        RFX_HIP(cp(out.ext_len, in.ext_len, (size_t)n * 4)); RFX_HIP(cp(out.marker, in.marker, (size_t)n * 4));
        RFX_HIP(cp(out.left, in.left, (size_t)n * 4)); RFX_HIP(cp(out.right, in.right, (size_t)n * 4));
        return RFX_OK;
    }
    DevBuf ps;
    uint32_t lmin = 0;
    const DynDev *cur = &in;
    for (int it = 0; it < rounds; it++) {
        DynDev s;
        RFX_TRY(dyn_sort(ctx, *cur, P, s, ps, &lmin));
        RFX_TRY(dyn_pass(ctx, s, ps.as<int64_t>(), P, lmin, 1, 5, start_marker, out, nullptr));
        RFX_TRY(sync_checked(ctx));                               // (s and the pass's temporaries are read until here)
        cur = &out;
    }
    return RFX_OK;
}

// step 3, first half: which contigs are kept and what they take
int rfx::fx2_contigs_plan(rfx_ctx *ctx, const DynDev &in, int max_k, Fx2Plan &plan) {
    const int64_t n = in.n;
    plan.m = 0; plan.words = 0;
    if (n == 0) return RFX_OK;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "contig fixing, round two: 2^31 records or more"; return RFX_E_LIMIT; }
    DevBuf nw, flags;
    RFX_ALLOC(plan.keep, uint32_t, n); RFX_ALLOC(nw, uint32_t, n);
    RFX_ALLOC(plan.rank, uint64_t, n + 1); RFX_ALLOC(plan.woff, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_fx2_cat_sizes, n, in.key_len.as<uint8_t>(), in.ext_len.as<int32_t>(), n, 2 * max_k,
                 plan.keep.as<uint32_t>(), nw.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, plan.keep.as<uint32_t>(), nw.as<uint32_t>(), plan.rank.as<uint64_t>(), plan.woff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, plan.rank.as<uint64_t>() + n, plan.woff.as<uint64_t>() + n, nullptr, &f));
    if (f.bad & FX2_BAD_EXT) { ctx->last_error = "contig fixing, round two: a negative extension length"; return RFX_E_ARG; }
    if (f.bad & FX2_TOO_LONG) { ctx->last_error = "contig fixing, round two: a contig of 2^30 bases or more"; return RFX_E_LIMIT; }
    plan.m = (int64_t)f.total[0]; plan.words = (int64_t)f.total[1];
    return RFX_OK;
}
// second half: the kept contigs into arrays that hold plan.m contigs (word_off: plan.m + 1) and plan.words words
int rfx::fx2_contigs_fill(rfx_ctx *ctx, const DynDev &in, const Fx2Plan &plan, uint64_t *d_words, int64_t *d_word_off, int64_t *d_len, int32_t *d_left,
                          int32_t *d_right) {
    const int64_t n = in.n;
    if (n == 0 || plan.m == 0) {
        RFX_HIP(hipMemsetAsync(d_word_off, 0, 8, ctx->stream));
        return RFX_OK;
    }
    RFX_LAUNCH_N(k_fx2_cat, n + plan.words, dyn_view(in), n, plan.keep.as<uint32_t>(), plan.rank.as<uint64_t>(),
                 plan.woff.as<uint64_t>(), d_words, d_word_off, d_len, d_left, d_right);
    return RFX_OK;
}

// steps 4-5: 05FixingAgain (ends 0), 06ContigEnds (ends 1) or 09ExtendAgain (ends 2: v.left / v.right are not read) into d_text (filled up to cap, nothing at or past it); *total = the text's
// length; own: a buffer of the library's, as long as the text
int rfx::fx2_text(rfx_ctx *ctx, const Fx2View &v, int ends, char *d_text, int64_t cap, int64_t *total, DevBuf *own) {
    const int64_t n = v.n;
    *total = 0;
    if (n == 0) return RFX_OK;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "contig fixing, round two: 2^31 contigs or more"; return RFX_E_LIMIT; }
    DevBuf sz, toff, flags;
    RFX_ALLOC(sz, uint64_t, n); RFX_ALLOC(toff, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_fx2_text_sizes, n, v.woff, v.len, v.left, v.right, n, ends, sz.as<uint64_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u64(ctx, sz.as<uint64_t>(), toff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, toff.as<uint64_t>() + n, nullptr, nullptr, &f));
    if (f.bad & FX2_BAD_LAYOUT) { ctx->last_error = "contigs: word_off and len disagree (word_off[0] = 0, word_off[i+1] - word_off[i] = (len[i] + 31) / 32)"; return RFX_E_ARG; }
    if (f.bad & FX2_TOO_LONG) { ctx->last_error = "contig fixing, round two: a contig of 2^30 bases or more"; return RFX_E_LIMIT; }
    if (f.bad & FX2_LINE_BREAK) { ctx->last_error = "contig extension, round two: a contig of 10,000,000 bases or more"; return RFX_E_LIMIT; }
    *total = (int64_t)f.total[0];
    if (own) {
        RFX_HIP(own->alloc((size_t)std::max<int64_t>(*total, 1), ctx->stream));
        d_text = own->as<char>(); cap = *total;
    }
    const int64_t lim = std::min<int64_t>(*total, cap);
    if (lim > 0) {
        const int skew = (int)((uintptr_t)d_text & 15);
        const int64_t chunks = ceil_div(lim + skew, 16);
        RFX_LAUNCH_N(k_fx2_text_fill, chunks, v.w, v.woff, v.len, v.left, v.right, n, ends, toff.as<uint64_t>(), lim, skew, chunks,
                     d_text);
    }
    return sync_checked(ctx);
}

// ---- the entry points, and what those of the later stages on contig sets share with them (rfx_internal.h) ------------------------------
bool rfx::fx2_contigs_ok(const rfx_contigs_packed *p) { return p && p->words && p->word_off && p->len; }
bool rfx::fx2_contigs_in_ok(const rfx_contigs_packed *p, const int32_t *d_left, const int32_t *d_right) {
    return fx2_contigs_ok(p) && p->n >= 0 && (p->n == 0 || (d_left && d_right));
}
int rfx::fx2_params(rfx_ctx *ctx, const rfx_fix_params *p, int P, const char *stage) {
    if (!p || !parts_ok(P)) return RFX_E_ARG;
    if (p->max_k < 31 || p->max_k > 124) { ctx->last_error = std::string(stage) + ": max_k must be 31..124"; return RFX_E_ARG; }
    if (p->max_iteration < -1) { ctx->last_error = std::string(stage) + ": max_iteration below -1"; return RFX_E_ARG; }
    return RFX_OK;
}
int rfx::fx2_text_call(rfx_ctx *ctx, int ends, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, char *d_text, int64_t cap,
                       int64_t *out_len) {
    if (!ctx || !fx2_contigs_ok(d_in) || d_in->n < 0 || (ends != 2 && d_in->n > 0 && (!d_left || !d_right)) || !text_out_ok(d_text, cap, out_len))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    int64_t total = 0;
    RFX_TRY(fx2_text(ctx, fx2_view(d_in, d_left, d_right), ends, d_text, cap, &total, nullptr));
    *out_len = total;
    return total > cap ? RFX_E_CAP : RFX_OK;
}
int rfx::fx2_contigs_of_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, CtgDev &c) {
    DevBuf d_text, d_off;
    DynDev a, b;
    Fx2Plan plan;
    RFX_TRY(dyn_upload_text(ctx, text, row_off, n_rows, d_text, d_off));
    RFX_TRY(fx2_binarize(ctx, (const char *)d_text.p, d_off.as<int64_t>(), n_rows, a));
    RFX_TRY(fx2_run(ctx, a, P, params->scramble, params->max_iteration, b));
    RFX_TRY(fx2_contigs_plan(ctx, b, params->max_k, plan));
    RFX_TRY(ctg_alloc(ctx, c, plan.m, plan.words));
    return fx2_contigs_fill(ctx, b, plan, c.w.as<uint64_t>(), c.woff.as<int64_t>(), c.len.as<int64_t>(), c.left.as<int32_t>(), c.right.as<int32_t>());
}

extern "C" {

int rfx_dev_fix2_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_out) || !text_rows_ok(d_text, d_row_off, n_rows)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    RFX_TRY(fx2_binarize(ctx, d_text, d_row_off, n_rows, a));
    return dyn_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_fix2_run(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, const rfx_fix_params *params, rfx_dyn_packed *d_out) try {
    if (!ctx || !dyn_packed_out_ok(d_in) || d_in->n < 0 || !dyn_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, P));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a, b;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(fx2_run(ctx, a, P, params->scramble, params->max_iteration, b));
    return dyn_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_fix2_contigs(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_fix_params *params, rfx_contigs_packed *d_out, int32_t *d_left,
                         int32_t *d_right) try {
    if (!ctx || !dyn_packed_out_ok(d_in) || d_in->n < 0 || !fx2_contigs_ok(d_out) || !d_left || !d_right) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, 1));
    RFX_HIP(hipSetDevice(ctx->device));
    DynDev a;
    Fx2Plan plan;
    RFX_TRY(dyn_borrow(ctx, d_in, a));
    RFX_TRY(fx2_contigs_plan(ctx, a, params->max_k, plan));
    if (!packed_out_fits(d_out, plan.m, plan.words)) return RFX_E_CAP;
    RFX_TRY(fx2_contigs_fill(ctx, a, plan, d_out->words, d_out->word_off, d_out->len, d_left, d_right));
    d_out->n = plan.m;
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

int rfx_dev_fix2_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, char *d_text, int64_t cap,
                         int64_t *out_len) try {
    return fx2_text_call(ctx, 0, d_in, d_left, d_right, d_text, cap, out_len);
} RFX_API_CATCH(ctx)

int rfx_dev_fix2_ends_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, char *d_text, int64_t cap,
                           int64_t *out_len) try {
    return fx2_text_call(ctx, 1, d_in, d_left, d_right, d_text, cap, out_len);
} RFX_API_CATCH(ctx)

// host text in, both host texts out; everything between packed and in HBM: one upload, binarize, run, the contigs, both texts, one
// copy back each.  A short buffer: RFX_E_CAP with BOTH lengths set and NEITHER buffer written
int rfx_fix2_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                  int64_t *out_len, char *ends_out, int64_t ends_cap, int64_t *ends_len) try {
    if (!ctx || !text_rows_ok(text, row_off, n_rows) || !text_out_ok(out, cap, out_len) || !text_out_ok(ends_out, ends_cap, ends_len)) return RFX_E_ARG;
    RFX_TRY(fx2_params(ctx, params, P));
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_rows, d_ends;
    CtgDev c;
    int64_t t_rows = 0, t_ends = 0;
    RFX_TRY(fx2_contigs_of_text(ctx, text, row_off, n_rows, P, params, c));
    RFX_TRY(fx2_text(ctx, fx2_view(c), 0, nullptr, 0, &t_rows, &d_rows));
    RFX_TRY(fx2_text(ctx, fx2_view(c), 1, nullptr, 0, &t_ends, &d_ends));
    return text_to_host(ctx, {{d_rows, t_rows, out, cap, out_len}, {d_ends, t_ends, ends_out, ends_cap, ends_len}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"
