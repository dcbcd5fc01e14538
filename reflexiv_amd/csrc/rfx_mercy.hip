// rfx_mercy.hip -- the mercy k-mer stage (Count_<k>_mercy) on the 2-bit read store in HBM:
// P/ReflexivDSDynamicMercyKmer.java `assemblyFromKmer` (:157-322).  In -sensitive mode the reference scans every read again behind the
// counter, finds the windows whose k-mer survived the coverage filter (the SOLID k-mers) and rescues, with count 1, the k-mers of the
// holes between two such windows of one read.  Its four shuffles over one row per k-mer instance become a lookup per window here:
//   index        the solid keys are the counter's output, ascending: a check in a launch of its own (strictly ascending, below 4^k), its
//                bits read back before anything indexes with them; then a directory over the top b bits of the keys, 2^b + 1 offsets, b
//                from n so that a bucket holds about one key.  A lookup is two neighbouring offsets and a binary search INSIDE the bucket:
//                one probe for the usual bucket, log2 of its length for a long one (the poly-A neighbourhood).  No atomics, no hashing
//   scan         a WAVE per read, 64 windows a round: lanes 0..2 load the round's three words, every lane cuts its window out of two of
//                them (a shuffle and pk_seg32's two shifts), turns it round (pk_rev2), takes the smaller and looks it up -- 64
//                independent loads in flight; __ballot of the result IS the hit mask.  The lane of a hit owns the gap in FRONT of it: the
//                distance to the previous set bit of the mask, or to the last hit of an earlier round (one carried int)
//   two passes   count: the kept gaps' lengths added up per read; a scan; ONE read-back of the error bits and the total; fill: the same
//                kernel over the reads that have something (the others cost one load), every kept gap written by the whole wave at the
//                read's offset -- gaps in position order, so the rows come out in (read, position) order with no sort.  A lane cannot
//                write its own window at its rank, as one would wish: whether a window is kept is known only at the NEXT hit, which may
//                be rounds away, so the owner of the gap hands it to the wave when it is found (kept gaps are rare: holes of coverage)
//   text         rows of k + 3 bytes need no scan: one thread per 16-byte chunk cut at the destination ADDRESS, letters by pk_letters16
// DEVIATIONS, all stated: (1) one call handles ONE k.  (2) The count column of a solid row is not read; the reference parses it and
// drops it.  (3) The reference's RamenReadRangeCal throws on an empty partition; here an empty input gives an empty output.  (4)
// rfx_mercy_text sorts the count rows itself (and merges equal ones); rfx_dev_mercy_kmers requires the keys ascending, as the counter
// returns them.
#include <algorithm>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

namespace {

#define MC_BLOCK 256
#define MC_WAVES (MC_BLOCK / 64)
#define MC_DIR_BITS 26               // the directory's most: 2^26 + 1 offsets of 4 bytes (256 MB, for 2^26 solid keys or more)
#define MC_MAX_LEN PK_CLAMP          // the reference clamps a window index at 30000: a read that long is refused
#define MC_MAX_WPR 937               // words_per_read of the device entry point: no read of 30000 bases fits
#define MC_MAX_CLIP (1 << 20)        // a clip above any read length acts like this one (and keeps the int arithmetic in range)

// what is wrong with a call's input (CallFlags::bad)
enum { MC_BAD_SOLID = 1, MC_BAD_READ = 2, MC_BAD_OFFSETS = 4, MC_BAD_COMMA = 8, MC_BAD_COUNT = 16 };

struct McIndex { const uint64_t *keys; const uint32_t *dir; int64_t n; int shift; };
struct McReads { const uint64_t *w; const uint32_t *len; int64_t n; int wpr, k, fc, ec; };

// ---- index ---------------------------------------------------------------------------------------------------------------------------
// one thread per solid key, in a launch of its own BEFORE the directory is built from them: strictly ascending, below 4^k
__global__ __launch_bounds__(256) void k_mc_check(const uint64_t *__restrict__ keys, int64_t n, int k, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = keys[i];
    if ((v >> (2 * k)) != 0ull || (i > 0 && keys[i - 1] >= v)) atomicOr(&flags->bad, (uint32_t)MC_BAD_SOLID);
}
// dir[j] = the keys whose top bits are below j, j = 0..2^b: thread i (0..n) writes the entries between the bucket of key i - 1 and the
// bucket of key i, for which key i is the first that is not below them; thread n the rest.  Every entry is written once, by one thread
__global__ __launch_bounds__(256) void k_mc_dir(const uint64_t *__restrict__ keys, int64_t n, int shift, int64_t buckets, uint32_t *__restrict__ dir) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const int64_t lo = i > 0 ? (int64_t)(keys[i - 1] >> shift) + 1 : 0;
    const int64_t hi = i < n ? (int64_t)(keys[i] >> shift) : buckets;
    for (int64_t j = lo; j <= hi; j++) dir[j] = (uint32_t)i;
}
// is `key` (below 4^k) a solid k-mer: its bucket's two offsets, then a binary search that stays inside the bucket
__device__ __forceinline__ bool mc_solid(const McIndex &ix, uint64_t key) {
    const uint64_t b = key >> ix.shift;
    uint32_t lo = ix.dir[b], hi = ix.dir[b + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = ix.keys[mid];
        if (v == key) return true;
        if (v < key) lo = mid + 1; else hi = mid;
    }
    return false;
}
// a window at the front of a word (its k bases, zeros behind) -> the smaller of the k-mer and its reverse complement, as the counter's key
__device__ __forceinline__ uint64_t mc_canon(uint64_t front, int k) {
    const uint64_t fw = front >> (64 - 2 * k);
    const uint64_t rc = ~pk_rev2(front) & ((1ull << (2 * k)) - 1);          // turned round it sits at the back; the complement of its bits only
    return fw < rc ? fw : rc;
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------------
// A wave per read.  !FILL: cnt[i] = the mercy k-mers of read i.  FILL: they are written from off[i] on, in position order.
// A read gives nothing when it has no window behind its clips, when len - 15 - end_clip <= 1 (FastqTuple2Dataset's filter, whose 15 is
// fixed), or when it has 32 bases or more and its first 31 are A (its first block is 0: ExtractMercyKmerFromRead :932 takes it for a
// marker row).  A hit is a window p, front_clip <= p <= len - end_clip - k, whose canonical k-mer is solid; for neighbouring hits a < b
// the gap g = b - a - 1 is kept iff g >= 1 and not k - 1 <= g <= k + 1 (the footprint of one substitution, :1336)
template <bool FILL>
__global__ __launch_bounds__(MC_BLOCK) void k_mc_scan(const McReads rd, const McIndex ix, uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off,
                                                      uint64_t *__restrict__ out, CallFlags *__restrict__ flags) {
    const int lane = (int)(threadIdx.x & 63), k = rd.k;
    const int64_t nw = (int64_t)gridDim.x * MC_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * MC_WAVES + (threadIdx.x >> 6); i < rd.n; i += nw) {
        uint64_t at = 0;
        if (FILL) { at = off[i]; if (off[i + 1] == at) continue; }
        const uint32_t n32 = rd.len[i];
        if (n32 > 32u * (uint32_t)rd.wpr || n32 >= (uint32_t)MC_MAX_LEN) {       // the words do not hold it, or an index would be clamped: the call fails
            if (!FILL && lane == 0) { atomicOr(&flags->bad, (uint32_t)MC_BAD_READ); cnt[i] = 0u; }
            continue;
        }
        const int n = (int)n32, last = n - rd.ec - k;
        const uint64_t *rw = rd.w + i * rd.wpr;
        const bool none = last < rd.fc || n - 15 - rd.ec <= 1 || (n >= 32 && (rw[0] >> 2) == 0ull);
        uint32_t total = 0u;
        int prev = -1;                                                  // the last hit of the rounds behind
        if (!none) for (int r = rd.fc >> 6; r <= last >> 6; r++) {
            // the round's windows 64 r .. 64 r + 63 lie in words 2 r .. 2 r + 2 (a word past a window's last base is never used)
            const int wi = 2 * r + lane;
            const uint64_t x = lane < 3 && wi < rd.wpr ? rw[wi] : 0ull;
            const int h = lane >> 5, s = (lane & 31) * 2, p = 64 * r + lane;
            const uint64_t a = __shfl(x, h, 64), b = __shfl(x, h + 1, 64);
            const uint64_t cn = mc_canon(pk_keep((a << s) | (s ? b >> (64 - s) : 0ull), k), k);
            const bool hit = p >= rd.fc && p <= last && mc_solid(ix, cn);
            const uint64_t m = __ballot(hit);
            // the gap in front of a hit: back to the previous set bit, or to the last hit of an earlier round
            const uint64_t below = m & ((1ull << lane) - 1ull);
            const int from = below ? 64 * r + 63 - __clzll((long long)below) : prev;
            const int g = p - from - 1;
            const bool kept = hit && from >= 0 && g >= 1 && !(g >= k - 1 && g <= k + 1);
            for (uint64_t t = __ballot(kept); t; t &= t - 1ull) {       // (wave-uniform: every lane walks the same bits)
                const int owner = __ffsll((long long)t) - 1;
                const int ga = __shfl(from, owner, 64), gg = __shfl(g, owner, 64);
                if (FILL) {
                    for (int j = lane; j < gg; j += 64) out[at + (uint64_t)j] = mc_canon(pk_keep(pk_seg32(rw, n, ga + 1 + j), k), k);
                    at += (uint64_t)gg;
                } else {
                    total += (uint32_t)gg;
                }
            }
            if (m) prev = 64 * r + 63 - __clzll((long long)m);
        }
        if (!FILL && lane == 0) cnt[i] = total;
    }
}

// ---- text: the rows "KMER,1\n" -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mc_row_off(int64_t n, int row, int64_t *__restrict__ row_off) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n) row_off[q] = q * row;
}
// one thread per 16-byte chunk of the destination (k_ee_text_fill): chunk ch holds the text's bytes [16 ch - skew, 16 ch - skew + 16)
// cut to [0, lim), skew = the destination address mod 16, so a whole chunk is a 16-byte-aligned store.  Byte b is byte b % (k + 3) of
// row b / (k + 3)
__global__ __launch_bounds__(256) void k_mc_text(const uint64_t *__restrict__ keys, int k, int64_t lim, int skew, int64_t chunks, char *__restrict__ out) {
    const int64_t ch = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= chunks) return;
    const int64_t start = 16 * ch - skew;
    const int64_t b0 = start < 0 ? 0 : start, b1 = start + 16 < lim ? start + 16 : lim;
    const bool whole = b1 - b0 == 16;
    const int row = k + 3;
    int64_t i = b0 / row;
    int q = (int)(b0 - i * row);
    uint64_t key = keys[i] << (64 - 2 * k);                        // the k-mer at the front of a word
    uint32_t o0 = 0u, o1 = 0u, o2 = 0u, o3 = 0u;
    if (whole && q + 16 <= k) {
        const uint64_t x[1] = {key << (2 * q)};
        const Pk16 y = pk_letters16(x, 0);
        o0 = y.a; o1 = y.b; o2 = y.c; o3 = y.d;
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (b0 + j < b1) {
                if (q == row) { i++; q = 0; key = keys[i] << (64 - 2 * k); }
                const uint32_t cc = q < k ? pk_letter((uint32_t)(key >> (62 - 2 * q)) & 3u) : q == k ? (uint32_t)',' : q == k + 1 ? (uint32_t)'1' : (uint32_t)'\n';
                const uint32_t x = cc << (8 * (j & 3));
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

// ---- the count rows of the host form -------------------------------------------------------------------------------------------------
// One thread per row, read as k_ks_bin_sizes (rfx_ksort.hip) reads it: the row ends ahead of its trailing newline; the first ',' cuts
// it; a leading '(' of the k-mer and a trailing ')' of the count are dropped; the count must be 1 or more decimal digits (its value is
// not used).  keep = the k-mer has k letters; val = its key (A0 C1 G2, anything else 3)
__global__ __launch_bounds__(256) void k_mc_rows(const char *__restrict__ text, const int64_t *__restrict__ row_off, int64_t n, int k,
                                                 uint32_t *__restrict__ keep, uint64_t *__restrict__ val, CallFlags *__restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int64_t b = row_off[r], e = row_off[r + 1];
    uint32_t bad = 0u, kp = 0u;
    uint64_t v = 0ull;
    if (e < b || b < 0) { bad |= MC_BAD_OFFSETS; e = b = 0; }
    while (e > b && (text[e - 1] == '\n' || text[e - 1] == '\r')) e--;
    int64_t c = b;
    while (c < e && text[c] != ',') c++;
    if (c >= e) bad |= bad ? 0u : (uint32_t)MC_BAD_COMMA;
    else {
        int64_t kb = b, ce = e;
        if (kb < c && text[kb] == '(') kb++;
        if (ce > c + 1 && text[ce - 1] == ')') ce--;
        bool digits = ce > c + 1;
        for (int64_t i = c + 1; i < ce; i++) if (text[i] < '0' || text[i] > '9') { digits = false; break; }
        if (!digits) bad |= MC_BAD_COUNT;
        if (c - kb == k) {
            kp = 1u;
            for (int j = 0; j < k; j++) v = (v << 2) | pk_code(text[kb + j]);
        }
    }
    keep[r] = bad ? 0u : kp;
    val[r] = v;
    if (bad) atomicOr(&flags->bad, bad);
}
// the kept of n values, in order (rank: the scan of keep)
__global__ __launch_bounds__(256) void k_mc_compact(const uint64_t *__restrict__ in, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ rank,
                                                    int64_t n, uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && keep[i]) out[rank[i]] = in[i];
}
// the first of every run of equal values of a sorted array
__global__ __launch_bounds__(256) void k_mc_heads(const uint64_t *__restrict__ in, int64_t n, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keep[i] = i == 0 || in[i - 1] != in[i] ? 1u : 0u;
}

int mc_bad(rfx_ctx *ctx, uint32_t bad) {
    if (!bad) return RFX_OK;
    ctx->last_error = bad & MC_BAD_SOLID   ? "mercy k-mers: solid keys that are not strictly ascending or not below 4^k"
                    : bad & MC_BAD_READ    ? "mercy k-mers: a read longer than 32 * words_per_read bases, or of 30000 bases or more"
                    : bad & MC_BAD_OFFSETS ? "mercy k-mers: row offsets that run backwards"
                    : bad & MC_BAD_COMMA   ? "mercy k-mers: a count row without a comma"
                                           : "mercy k-mers: a count that is not decimal digits";
    return RFX_E_ARG;
}

// what one call keeps between its two passes
struct McPlan { int64_t total = 0; int shift = 0; DevBuf dir, cnt, off; };

// the index, the counting pass and the scan of its counts: plan.total = the mercy k-mers of the call
int mc_plan(rfx_ctx *ctx, const uint64_t *d_solid, int64_t n_solid, const McReads &rd, McPlan &plan) {
    plan.total = 0;
    if (n_solid >= ((int64_t)1 << 31) || rd.n >= ((int64_t)1 << 31)) { ctx->last_error = "mercy k-mers: 2^31 solid keys or reads, or more"; return RFX_E_LIMIT; }
    DevBuf flags;
    CallFlags f{};
    RFX_TRY(call_flags_init(ctx, flags));
    if (n_solid > 0) {
        RFX_LAUNCH_N(k_mc_check, n_solid, d_solid, n_solid, rd.k, flags.as<CallFlags>());
        RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));      // (refused keys are not indexed with)
        RFX_TRY(mc_bad(ctx, f.bad));
    }
    int b = 1;
    while (b < std::min(2 * rd.k, MC_DIR_BITS) && ((int64_t)1 << b) < n_solid) b++;
    plan.shift = 2 * rd.k - b;
    const int64_t buckets = (int64_t)1 << b;
    RFX_ALLOC(plan.dir, uint32_t, buckets + 1);
    RFX_LAUNCH_N(k_mc_dir, n_solid + 1, d_solid, n_solid, plan.shift, buckets, plan.dir.as<uint32_t>());
    RFX_ALLOC(plan.cnt, uint32_t, std::max<int64_t>(rd.n, 1)); RFX_ALLOC(plan.off, uint64_t, rd.n + 1);
    if (rd.n == 0) return sync_checked(ctx);
    const McIndex ix{d_solid, plan.dir.as<uint32_t>(), n_solid, plan.shift};
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(rd.n, MC_WAVES), 8 * (int64_t)std::max(ctx->num_cu, 1));
    RFX_LAUNCH(k_mc_scan<false>, dim3(grid), dim3(MC_BLOCK), 0, rd, ix, plan.cnt.as<uint32_t>(), nullptr, nullptr, flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, plan.cnt.as<uint32_t>(), plan.off.as<uint64_t>(), rd.n));
    RFX_TRY(call_flags_read(ctx, flags, plan.off.as<uint64_t>() + rd.n, nullptr, nullptr, &f));
    RFX_TRY(mc_bad(ctx, f.bad));
    if (f.total[0] >= ((uint64_t)1 << 31)) { ctx->last_error = "mercy k-mers: 2^31 mercy k-mers or more"; return RFX_E_LIMIT; }
    plan.total = (int64_t)f.total[0];
    return RFX_OK;
}
// the mercy k-mers into an array that holds plan.total of them
int mc_fill(rfx_ctx *ctx, const uint64_t *d_solid, int64_t n_solid, const McReads &rd, const McPlan &plan, uint64_t *d_out) {
    if (plan.total == 0) return RFX_OK;
    const McIndex ix{d_solid, plan.dir.as<uint32_t>(), n_solid, plan.shift};
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(rd.n, MC_WAVES), 8 * (int64_t)std::max(ctx->num_cu, 1));
    RFX_LAUNCH(k_mc_scan<true>, dim3(grid), dim3(MC_BLOCK), 0, rd, ix, nullptr, plan.off.as<uint64_t>(), d_out, nullptr);
    return RFX_OK;
}
// the rows "KMER,1\n" of n keys into d_text (filled up to cap, nothing at or past it) and their n + 1 offsets into d_row_off (nullptr:
// none); *total = the text's length; own: a buffer of the library's
int mc_text(rfx_ctx *ctx, const uint64_t *d_keys, int64_t n, int k, char *d_text, int64_t cap, int64_t *total, int64_t *d_row_off, DevBuf *own) {
    *total = n * (k + 3);
    if (own) {
        RFX_HIP(own->alloc((size_t)std::max<int64_t>(*total, 1), ctx->stream));
        d_text = own->as<char>(); cap = *total;
    }
    if (d_row_off) RFX_LAUNCH_N(k_mc_row_off, n + 1, n, k + 3, d_row_off);
    const int64_t lim = std::min<int64_t>(*total, cap);
    if (lim > 0) {
        const int skew = (int)((uintptr_t)d_text & 15);
        const int64_t chunks = ceil_div(lim + skew, 16);
        RFX_LAUNCH_N(k_mc_text, chunks, d_keys, k, lim, skew, chunks, d_text);
    }
    return sync_checked(ctx);
}
bool mc_args_ok(rfx_ctx *ctx, int k, int front_clip, int end_clip) {
    if (k < 8 || k > 31) { ctx->last_error = "mercy k-mers: k must be 8..31"; return false; }
    if (front_clip < 0 || end_clip < 0) { ctx->last_error = "mercy k-mers: a negative clip"; return false; }
    return true;
}

}  // namespace

// ---- the entry points ------------------------------------------------------------------------------------------------------------
extern "C" {

int rfx_dev_mercy_kmers(rfx_ctx *ctx, const uint64_t *d_solid_keys, int64_t n_solid, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads,
                        int words_per_read, int k, int front_clip, int end_clip, uint64_t *d_out_keys, int64_t cap, int64_t *out_n) try {
    if (!ctx || !out_n || n_solid < 0 || n_reads < 0 || cap < 0 || (n_solid > 0 && !d_solid_keys) || (n_reads > 0 && (!d_words || !d_read_len)) ||
        (cap > 0 && !d_out_keys) || !mc_args_ok(ctx, k, front_clip, end_clip))
        return RFX_E_ARG;
    if (words_per_read < 1 || words_per_read > MC_MAX_WPR) { ctx->last_error = "mercy k-mers: words_per_read must be 1..937"; return RFX_E_ARG; }
    RFX_HIP(hipSetDevice(ctx->device));
    const McReads rd{d_words, d_read_len, n_reads, words_per_read, k, std::min(front_clip, MC_MAX_CLIP), std::min(end_clip, MC_MAX_CLIP)};
    McPlan plan;
    RFX_TRY(mc_plan(ctx, d_solid_keys, n_solid, rd, plan));
    if (plan.total > cap) { *out_n = plan.total; return RFX_E_CAP; }
    RFX_TRY(mc_fill(ctx, d_solid_keys, n_solid, rd, plan, d_out_keys));
    RFX_TRY(sync_checked(ctx));
    *out_n = plan.total;
    return RFX_OK;
} RFX_API_CATCH(ctx)

int rfx_dev_mercy_to_text(rfx_ctx *ctx, const uint64_t *d_keys, int64_t n, int k, char *d_text, int64_t cap, int64_t *out_len, int64_t *d_row_off) try {
    if (!ctx || n < 0 || (n > 0 && !d_keys) || !text_out_ok(d_text, cap, out_len) || !mc_args_ok(ctx, k, 0, 0)) return RFX_E_ARG;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "mercy k-mers: 2^31 mercy k-mers or more"; return RFX_E_LIMIT; }
    RFX_HIP(hipSetDevice(ctx->device));
    int64_t total = 0;
    RFX_TRY(mc_text(ctx, d_keys, n, k, d_text, cap, &total, d_row_off, nullptr));
    *out_len = total;
    return total > cap ? RFX_E_CAP : RFX_OK;
} RFX_API_CATCH(ctx)

// host form: the rows of Count_<k> and ASCII reads in, the rows of Count_<k>_mercy out; everything between in HBM: one upload each, the
// solid keys parsed, sorted and made distinct, the read store, the index, both passes, the text, one copy back
int rfx_mercy_text(rfx_ctx *ctx, const char *count_text, const int64_t *count_row_off, int64_t n_rows, const uint8_t *bases, const int64_t *read_off,
                   int64_t n_reads, int k, int front_clip, int end_clip, char *out, int64_t cap, int64_t *out_len) try {
    if (!ctx || !text_rows_ok(count_text, count_row_off, n_rows) || !text_rows_ok((const char *)bases, read_off, n_reads) || !text_out_ok(out, cap, out_len) ||
        !mc_args_ok(ctx, k, front_clip, end_clip))
        return RFX_E_ARG;
    if (n_rows >= ((int64_t)1 << 31) || n_reads >= ((int64_t)1 << 31)) {          // (before an offset is read or a byte uploaded)
        ctx->last_error = "mercy k-mers: 2^31 count rows or reads, or more";
        return RFX_E_LIMIT;
    }
    int64_t longest = 1;
    for (int64_t i = 0; i < n_reads; i++) longest = std::max(longest, read_off[i + 1] - read_off[i]);
    if (longest >= MC_MAX_LEN) { ctx->last_error = "mercy k-mers: a read of 30000 bases or more"; return RFX_E_ARG; }
    RFX_HIP(hipSetDevice(ctx->device));
    const int wpr = (int)((longest + 31) >> 5);
    DevBuf d_ct, d_co, d_b, d_ro, d_words, d_len, d_rows, flags, keep, val, rank, keys, tk, tv, vals, solid, mercy;
    RFX_TRY(dyn_upload_text(ctx, count_text, count_row_off, n_rows, d_ct, d_co));
    RFX_TRY(dyn_upload_text(ctx, (const char *)bases, read_off, n_reads, d_b, d_ro));
    // the solid set: the rows of k letters as keys, sorted, one of each
    int64_t m = 0, n_solid = 0;
    const int64_t r1 = std::max<int64_t>(n_rows, 1);
    RFX_ALLOC(keep, uint32_t, r1); RFX_ALLOC(val, uint64_t, r1); RFX_ALLOC(rank, uint64_t, r1 + 1); RFX_ALLOC(solid, uint64_t, r1);
    if (n_rows > 0) {
        CallFlags f{};
        RFX_TRY(call_flags_init(ctx, flags));
        RFX_LAUNCH_N(k_mc_rows, n_rows, d_ct.as<char>(), d_co.as<int64_t>(), n_rows, k, keep.as<uint32_t>(), val.as<uint64_t>(), flags.as<CallFlags>());
        RFX_TRY(exclusive_scan_u32_to_u64(ctx, keep.as<uint32_t>(), rank.as<uint64_t>(), n_rows));
        RFX_TRY(call_flags_read(ctx, flags, rank.as<uint64_t>() + n_rows, nullptr, nullptr, &f));
        RFX_TRY(mc_bad(ctx, f.bad));
        m = (int64_t)f.total[0];
    }
    if (m > 0) {
        RFX_ALLOC(keys, uint64_t, m); RFX_ALLOC(tk, uint64_t, m); RFX_ALLOC(vals, uint32_t, m); RFX_ALLOC(tv, uint32_t, m);
        RFX_LAUNCH_N(k_mc_compact, n_rows, val.as<uint64_t>(), keep.as<uint32_t>(), rank.as<uint64_t>(), n_rows, keys.as<uint64_t>());
        RFX_HIP(hipMemsetAsync(vals.p, 0, (size_t)m * sizeof(uint32_t), ctx->stream));
        RFX_TRY(sort_pairs(ctx, keys.as<uint64_t>(), vals.as<uint32_t>(), m, 2 * k, tk.as<uint64_t>(), tv.as<uint32_t>()));
        RFX_LAUNCH_N(k_mc_heads, m, keys.as<uint64_t>(), m, keep.as<uint32_t>());
        RFX_TRY(scan_keep(ctx, keep.as<uint32_t>(), m, rank.as<uint64_t>(), &n_solid));
        RFX_LAUNCH_N(k_mc_compact, m, keys.as<uint64_t>(), keep.as<uint32_t>(), rank.as<uint64_t>(), m, solid.as<uint64_t>());
    }
    const int64_t n1 = std::max<int64_t>(n_reads, 1);
    RFX_ALLOC(d_words, uint64_t, n1 * wpr); RFX_ALLOC(d_len, uint32_t, n1);
    if (n_reads > 0) RFX_TRY(encode_reads(ctx, d_b.as<uint8_t>(), d_ro.as<int64_t>(), n_reads, wpr, d_words.as<uint64_t>(), d_len.as<uint32_t>()));
    const McReads rd{d_words.as<uint64_t>(), d_len.as<uint32_t>(), n_reads, wpr, k, std::min(front_clip, MC_MAX_CLIP), std::min(end_clip, MC_MAX_CLIP)};
    McPlan plan;
    RFX_TRY(mc_plan(ctx, solid.as<uint64_t>(), n_solid, rd, plan));
    RFX_ALLOC(mercy, uint64_t, std::max<int64_t>(plan.total, 1));
    RFX_TRY(mc_fill(ctx, solid.as<uint64_t>(), n_solid, rd, plan, mercy.as<uint64_t>()));
    int64_t total = 0;
    RFX_TRY(mc_text(ctx, mercy.as<uint64_t>(), plan.total, k, nullptr, 0, &total, nullptr, &d_rows));
    return text_to_host(ctx, {{d_rows, total, out, cap, out_len}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"
