// rfx_count.h -- what the count stage's translation units share.
//
//   rfx_kmer.hip      encoding, the 64-bit instance path, the later levels, every leaf, the W-word element path, the entry
//                     points (count_filter is the dispatcher of k <= 31)
//   rfx_count_sk.hip  level 1 of the record paths: reads -> super-k-mer records (two passes, or one sweep), by radix digit
//                     or by owner
// This header holds (1) the device-side types, constants and force-inlined helpers that kernels of both units use, and
// (2) the host functions that one unit defines and the other calls.  A kernel is never declared here: it is launched only
// from the unit that defines it.  Tuning constants of one kernel live next to that kernel.  MAX_BITS and the environment
// knobs are defined in rfx_count_tuning.h (host-only) and nowhere else.
#pragma once
#include "rfx_internal.h"
#include "rfx_device.h"
#include "rfx_count_tuning.h"
#include <type_traits>
#include <vector>

namespace rfxc {

using namespace rfxd;

// number of k-mers a read of length len emits (skip rule :3020, loop bounds :3027,:3050)
__device__ __host__ __forceinline__ int64_t nk_of(int64_t len, int k, int fc, int ec) {
    if (len - k - ec <= 1 || fc > len) return 0;
    int64_t m = (len - ec - fc) - (k - 1);
    return m > 0 ? m : 0;
}

// the same for the k > 31 counter (P/ReflexivDataFrameCounter64.java:410, nk_of_w in rfx_wide.hip): a read
// of length k (k + 1) emits one (two) k-mers there, none at k <= 31
__device__ __host__ __forceinline__ int64_t nk_of_wide(int64_t len, int k, int fc, int ec) {
    if (len - k - ec + 1 <= 0 || fc > len) return 0;
    int64_t m = (len - ec - fc) - (k - 1);
    return m > 0 ? m : 0;
}

constexpr int PK = 16;                // instances per thread

struct Level {
    int bits;                 // digit width of this level
    int shift;                // digit = (h >> shift) & (2^bits - 1); child id = h >> shift
    int parent_shift;         // parent id = h >> parent_shift (64 -> id 0)
    int n_owners;             // > 0: the "digit" is the owning rank, mulhi(kmer_hash, n_owners)
    int sub_bits;             // level 1 in one sweep by owner: digit = owner << sub_bits | the header's top sub_bits bits
                              // (bins = 2^bits, bits = ceil(log2(n_owners)) + sub_bits; see bucket_records_by_owner_sweep)
};

// A thread owns PK consecutive windows of ONE read ("segment"): it loads the <= 3 packed words
// they span, builds the first k-mer and its reverse complement with shifts and a bit reversal,
// and rolls both through the remaining windows in registers -- no LDS, no per-base loads.
struct ReadSrc {
    const uint64_t *words;
    int64_t n_reads, n_threads;    // n_threads = n_reads * segs
    int wpr, nk, fc, k, segs;      // words/read, k-mers/read (of the longest read), front clip, k, segments/read
    const uint32_t *len_arr;       // ragged reads: per-read length (nullptr: every read emits nk k-mers)
    int ec;                        // end clip (for the per-read count)
    int wfl;                       // k = 33..63 records: bases of the k-mer on either side of the central window (else 0)
};

// k-mers read r emits.  WIDE: a k = 33..63 source, whose k / fc describe the central window -- the k-mers are
// counted on the real k (k + 2 wfl) and front clip with the counter64 skip rule (a compile-time choice: the
// k <= 31 kernels carry none of it)
template <bool WIDE = false>
__device__ __forceinline__ int read_nk(const ReadSrc &s, int64_t r) {
    if constexpr (WIDE) return s.len_arr ? (int)nk_of_wide((int64_t)s.len_arr[r], s.k + 2 * s.wfl, s.fc - s.wfl, s.ec) : s.nk;
    return s.len_arr ? (int)nk_of((int64_t)s.len_arr[r], s.k, s.fc, s.ec) : s.nk;
}

struct SegPos { int64_t r; int sgm; };

template <int SEG = 16>
__device__ __forceinline__ void seg_load(const ReadSrc &s, const SegPos &q, uint64_t (&w)[3]) {
    const uint64_t *g = s.words + q.r * s.wpr;
    const int wi = (s.fc + q.sgm * SEG) >> 5;
    const int last = s.wpr - 1;
    w[0] = g[wi < last ? wi : last];
    w[1] = g[wi + 1 < last ? wi + 1 : last];
    w[2] = g[wi + 2 < last ? wi + 2 : last];
}

struct alignas(16) Rec { uint64_t w0, w1; };
// Rec: w0 = bases 0..31 of the run's base string, w1 = [63..36] bases 32..45, [35..32] windows-1,
// [31..0] the top 32 bits of the minimiser's local hash (radix digits peel off its top).
__device__ __forceinline__ int rec_len(const Rec &r) { return (int)((r.w1 >> 32) & 15) + 1; }
// WRec: the super-k-mer record of the k = 33..63 path.  b0..b2 = bases 0..95 of the run's base string (the
// run's first k-mer starts at base 0; k + windows - 1 <= 78 bases are used), hd = [35..32] windows-1,
// [31..0] the top 32 bits of the minimiser's local hash.  The minimiser is taken over the CENTRAL 31
// (k odd) or 30 (k even) bases of the k-mer, which the reverse complement maps onto themselves, so it
// is a function of the canonical k-mer as on the k <= 31 path -- and the front end is the k = 31 / 30 one.
struct alignas(32) WRec { uint64_t b0, b1, b2, hd; };
__device__ __forceinline__ int rec_len(const WRec &r) { return (int)((r.hd >> 32) & 15) + 1; }
__device__ __forceinline__ uint32_t rec_hdr(const Rec &r) { return (uint32_t)r.w1; }

// Record streams of the radix levels.  The last level's sweep (k_rec_l2sweep) touches every record once on the way in and once
// on the way out, 9 + 9 GB a step, and nothing of it is used again before the leaves stream it: both sides carry the
// non-temporal hint (`nt` on the global_load / global_store), so the stream does not take cache lines as if it were to be
// re-used.  (4.36 -> 3.8 ms; the hint on the loads alone is a loss, on the stores alone two thirds of
// the gain.)  Records move as native 16-byte vectors, one or two each.
// Level 1's sweep (k_sk_onesweep) writes its rings' lines the same way (section 30).
typedef unsigned long long l2_v2 __attribute__((ext_vector_type(2)));
template <class RT>
__device__ __forceinline__ RT l2_load_stream(const RT *p) {
    static_assert(sizeof(RT) == 16 || sizeof(RT) == 32, "16- or 32-byte records");
    const l2_v2 a = __builtin_nontemporal_load((const l2_v2 *)p);
    if constexpr (sizeof(RT) == 32) {
        const l2_v2 b = __builtin_nontemporal_load((const l2_v2 *)p + 1);
        return RT{a.x, a.y, b.x, b.y};
    } else return RT{a.x, a.y};
}
template <class RT>
__device__ __forceinline__ void l2_store_stream(RT *p, const RT &r) {
    const uint64_t *w = (const uint64_t *)&r;
    __builtin_nontemporal_store(l2_v2{w[0], w[1]}, (l2_v2 *)p);
    if constexpr (sizeof(RT) == 32) __builtin_nontemporal_store(l2_v2{w[2], w[3]}, (l2_v2 *)p + 1);
}

// super-k-mer records (rfx_count_sk.hip): runs of windows that share a minimiser, the canonical SK_M-mer with the smallest hash
constexpr int SK_M = 13;
constexpr int SK_MIN_W = 9;           // record path for k = 21..31 (W = k - 12 m-mers per window)
// super-k-mer records are used for k = 28..31 (W = k - 12 in 16..19)
inline bool superkmer_enabled(int k) {
    return k >= SK_M + SK_MIN_W - 1 && k <= 31;
}

// digit of a record at a level that follows `used` radix bits
__device__ __forceinline__ unsigned rec_digit(uint32_t hdr, int used, int bits) {
    return bits ? (unsigned)((hdr << used) >> (32 - bits)) : 0u;
}

}  // namespace rfxc

namespace rfx {

using namespace rfxc;
#pragma GCC visibility push(hidden)   // internal to the library: none of these is among its exported symbols

// ---- rfx_kmer.hip
// the radix plan for n instances: bits per level (RFX_LEVEL_BITS overrides, RFX_LEAF_TARGET replaces `target`)
void plan_levels(int64_t n, bool from_reads, std::vector<int> &bits, double target = 16384.0);
ReadSrc make_read_src(const ReadStore *reads);
int64_t instances_of(const ReadStore *reads, const ReadSrc &s);        // k-mer instances of a read set
int zero_owner_offsets(rfx_ctx *ctx, int n_owners, int64_t *d_owner_off, int64_t *h_owner_off);
// k_bin_offsets for the other unit's exact level 1 (a kernel is launched only from the unit that defines it)
int bin_offsets(rfx_ctx *ctx, const uint64_t *d_scanned, int nb, int64_t grid, uint64_t *d_seg_off);
// the levels behind level 1 and the record leaves
int count_records_levels(rfx_ctx *ctx, const Rec *recs, int64_t n_recs, int ws_slot_of_recs,
                         const std::vector<int> &bits, size_t first_level, int used, DevBuf *seg_cur,
                         DevBuf *seg_next, int64_t nseg, int k, int min_cov, int max_cov, int twin,
                         uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap, int64_t *out_n,
                         int64_t *out_distinct, bool pair_out = false, const uint64_t *seg_end_first = nullptr);

// ---- rfx_count_sk.hip (the two templates are instantiated there for WIDE = false, true)
template <bool WIDE = false>
int records_from_reads(rfx_ctx *ctx, const ReadSrc &rsrc, const Level &lv, bool use_ws, int ws_slot,
                       std::conditional_t<WIDE, WRec, Rec> *d_dst, int64_t cap_dst, uint64_t *d_seg_off,
                       std::conditional_t<WIDE, WRec, Rec> **out_recs, int64_t *n_recs, const char *hn, const char *pn);
template <bool WIDE = false>
int records_onesweep(rfx_ctx *ctx, const ReadSrc &rsrc_in, const Level &lv, int ws_slot, uint64_t *d_seg_begin,
                     uint64_t *d_seg_end, std::conditional_t<WIDE, WRec, Rec> **out_recs, int64_t *n_recs, bool *done,
                     const char *hn, const char *pn, std::conditional_t<WIDE, WRec, Rec> *d_dst = nullptr, int64_t cap_dst = 0);
int count_reads_superkmer(rfx_ctx *ctx, const ReadStore *reads, int min_cov, int max_cov, int twin, uint64_t *d_out_keys,
                          int32_t *d_out_counts, int64_t cap, int64_t *out_n, int64_t *out_distinct, bool pair_out);
ReadSrc wide_read_src(const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                      const uint32_t *d_read_len = nullptr, int ec = 0);

#pragma GCC visibility pop

}  // namespace rfx
