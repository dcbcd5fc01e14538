// rfx_count_sk.hip -- level 1 of the record paths: packed reads -> super-k-mer records, bucketed by a radix digit of the
// minimiser's hash or by the rank that owns it.  16-byte records (Rec) for k = 28..31, 32-byte records (WRec, WIDE) for
// k = 33..63, whose minimiser is taken over the k-mer's central 30 / 31 bases so that the same front end serves both.
//   seg_runs                        a thread's 16 or 32 windows of one read, cut into runs that share a minimiser
//   k_sk_hist, k_sk_scatter         the exact two-pass form (records_from_reads): per-workgroup histogram rows, one scan,
//                                   write-combining rings; run descriptors carry the minimisers from pass to pass
//   k_sk_sample_hist, k_plan_regions, k_sk_onesweep, k_fix_holes
//                                   the one-sweep form (records_onesweep): regions sized by a sampled histogram, extents
//                                   handed out by atomics, holes closed afterwards; void when a region runs out
//   k_close_gaps, owner_sweep       the one sweep bucketed by owner (the multi-GPU exchange's send side)
// and the entry points that start here: count_reads_superkmer (the default count at k = 28..31; the levels and leaves
// follow in rfx_kmer.hip: count_records_levels) and the bucket_*records_by_owner* calls.
#include "rfx_internal.h"
#include "rfx_device.h"
#include "rfx_count.h"
#include <algorithm>
#include <cmath>

using namespace rfxd;
using namespace rfxc;

namespace {

// ------------------------------------------------------- super-k-mer records

// Level 1 from reads, second form: instead of one 8-byte k-mer per window, a thread emits one
// 16-byte record per RUN of consecutive windows (inside its 16-window segment) that share a
// minimiser -- the canonical 13-mer with the smallest hash among the window's W = k-12 m-mers.
// The minimiser is a function of the canonical k-mer (the set of canonical m-mers is the same on
// both strands), so every instance of a k-mer follows the same bucket path; buckets are radix
// digits of the minimiser's hash.  ~6 windows per record -> ~2.6 B per instance through the
// partition levels instead of 8, and the leaf expands records straight into its LDS table, so the
// 8-byte instance array never exists in HBM.  (KMC / Gerbil-style, re-cut for wave64 + LDS.)
constexpr int SKT = 1024;             // threads per workgroup of the reads -> records kernels

// order of the m-mers: a bijection of the canonical 26-bit m-mer onto 32 bits (odd multiplier,
// xor-shift), so two different m-mers never tie and a plain 32-bit minimum picks the minimiser;
// the value itself (not the m-mer) names the bucket
// (round 3: ONE full-rate instruction, v_mad_u32_u24 -- the low 24 bits of the m-mer times a 24-bit odd
// constant, plus the m-mer (which brings in its first base, bits 24-25) -- instead of a quarter-rate 32-bit multiply, a
// shift and an xor: 34 m-mers per segment make this 15 % of level 1's issue cycles.  Not a bijection any more, and it need
// not be one: the value, not the m-mer, names the run and its bucket, so two m-mers that tie simply share a run -- the
// bucket is still a function of the canonical k-mer.)
__device__ __forceinline__ uint32_t mmer_key(uint32_t canon) { return __umul24(canon, 0x9E3779u) + canon; }

// Walks the runs of one segment; calls emit(first_window, n_windows, minimiser_key).
// SEG: windows per segment, 16 or 32 (round 3).  A thread that owns 32 windows evaluates 50 m-mers where two threads of 16
// evaluate 68, pays the per-segment work once, and -- what counts downstream -- a read is cut into records at half as
// many places that only depend on where the read happened to start: 19 % fewer records, and more of them identical from
// read to read.  Runs stay <= 16 windows (four bits in the record): a longer one is cut 16 windows after its start.
//
// SEG = 32 MERGES ACROSS SEGMENT EDGES.  Nine times in ten the minimiser does not change where a thread's 32 windows end,
// and the cut there is one more record for every level behind this one.  So the TAIL of a full segment (its last run after
// the 16-window cut, t windows) and the HEAD of the same read's next segment (its first run after the cut, b windows) are
// one run when their keys are equal: the tail's owner emits min(16, t + b) windows -- the cap counts from where the run
// started -- and the head starts that many minus t windows later, or is dropped when nothing is left of it.  A full
// segment has at least two runs (32 windows, none longer than 16), so head and tail are different runs and what a lane
// does never depends on more than its two neighbours.  Segments of a read are consecutive lanes: the four values (tail key
// and length, head key and length) and the bases past the thread's 64 (the top of the next lane's `lo`, *nx_out) are
// swapped with the neighbour lanes, and both lanes evaluate the same predicate on the same values.  Nothing merges across
// a wave's edge (a read of 5 segments straddles one; any cut is correct), and a segment without windows (ragged sets, the
// lanes past the last read) offers nothing.  EVERY LANE OF THE WAVE MUST CALL with SEG = 32 (nk_r = 0 where there is no
// segment): the exchange reads no register of an inactive lane.
// What holds in either form, and is all that the levels behind rely on:
//   * every window of every read lies in exactly one record;
//   * a record has 1..16 windows, all with the same minimiser key;
//   * the bucket is the hash of that key only.
// Which lane emits a record does not matter downstream.
template <int W, bool RUNLOOP, int SEG = 16, class F>
__device__ __forceinline__ void seg_runs(const ReadSrc &s, int nk_r, int sgm, const uint64_t (&w)[3], F &&emit,
                                         uint64_t *hi_out, uint64_t *lo_out, uint32_t *wm_lds = nullptr, uint32_t *nx_out = nullptr) {
    static_assert(SEG == 16 || SEG == 32, "segment");
    constexpr int PK = SEG;                        // (shadows the file-wide 16 inside this function)
    constexpr bool MERGE = SEG == 32;
    static_assert(!MERGE || RUNLOOP, "the merged cut walks the run-start bits");
    constexpr int NM = PK + W - 1;                 // m-mers a segment can touch (<= 34, or <= 50)
    static_assert(NM + SK_M - 1 <= 64, "the segment's bases lie in (hi, lo)");
    const int p0 = sgm * PK;
    int v = nk_r - p0;
    v = v > PK ? PK : v;
    if constexpr (MERGE) {
        v = v < 0 ? 0 : v;
        if (!__any(v > 0)) return;                 // (the same for the whole wave)
    } else if (v <= 0) return;                     // a short read of a ragged set: no window in this segment
    const int sh = 2 * ((s.fc + p0) & 31);
    const uint64_t hi = sh ? (w[0] << sh) | (w[1] >> (64 - sh)) : w[0];
    const uint64_t lo = sh ? (w[1] << sh) | (w[2] >> (64 - sh)) : w[1];
    *hi_out = hi; *lo_out = lo;
    constexpr int M2 = 2 * SK_M;
    const uint32_t mmask = (1u << M2) - 1;
    uint32_t val[NM];
    // Every m-mer is CUT out of the 64-base stream, and its reverse complement out of the stream's reverse complement
    // (made once: the complement of m-mer j is the m-mer at base 51 - j of it), at compile-time positions: a bit-field
    // extract when the 26 bits lie in one 32-bit word, a funnel shift and a shift otherwise -- 3.5 instructions for the
    // pair instead of the 6 of rolling both through a base at a time (rounds 1-2).
    static_assert(SK_M == 13 && NM <= 50, "positions below");
    const uint64_t rhi = revcomp(lo, 32), rlo = revcomp(hi, 32);
    const uint32_t FW[4] = {(uint32_t)(hi >> 32), (uint32_t)hi, (uint32_t)(lo >> 32), (uint32_t)lo};
    const uint32_t RW[4] = {(uint32_t)(rhi >> 32), (uint32_t)rhi, (uint32_t)(rlo >> 32), (uint32_t)rlo};
    auto cut = [&](const uint32_t (&Wd)[4], const int pos) __attribute__((always_inline)) -> uint32_t {
        const int wi = pos >> 4, off = 2 * (pos & 15);
        if (off + M2 <= 32) return (Wd[wi] >> (32 - M2 - off)) & mmask;
        return __builtin_amdgcn_alignbit(Wd[wi], Wd[wi < 3 ? wi + 1 : 3], 32 - off) >> (32 - M2);
    };
#pragma unroll
    for (int j = 0; j < NM; j++) {
        const uint32_t fm = cut(FW, j), rm = cut(RW, 64 - SK_M - j);
        val[j] = mmer_key(fm < rm ? fm : rm);
    }
    // per-window minimiser = sliding minimum over W m-mers (van Herk: suffix minima and prefix minima
    // inside blocks of W m-mers; a window spans at most two blocks)
    uint32_t wm[PK];
    if constexpr (W >= PK - 1) {
        // two blocks cover the segment: suffixes of [0, W) and prefixes of [W, NM), in place
#pragma unroll
        for (int j = W - 2; j >= 0; j--) val[j] = val[j] < val[j + 1] ? val[j] : val[j + 1];
#pragma unroll
        for (int j = W + 1; j < NM; j++) val[j] = val[j] < val[j - 1] ? val[j] : val[j - 1];
        wm[0] = val[0];
#pragma unroll
        for (int i = 1; i < PK; i++) wm[i] = val[i] < val[W + i - 1] ? val[i] : val[W + i - 1];
    } else {
        uint32_t sfx[NM], pfx[NM];
#pragma unroll
        for (int j = NM - 1; j >= 0; j--)
            sfx[j] = (j % W == W - 1 || j == NM - 1) ? val[j] : (val[j] < sfx[j + 1] ? val[j] : sfx[j + 1]);
#pragma unroll
        for (int j = 0; j < NM; j++) pfx[j] = (j % W == 0) ? val[j] : (val[j] < pfx[j - 1] ? val[j] : pfx[j - 1]);
#pragma unroll
        for (int i = 0; i < PK; i++) wm[i] = sfx[i] < pfx[i + W - 1] ? sfx[i] : pfx[i + W - 1];
    }
    if constexpr (!RUNLOOP) {
        // cheap emit(): call it where the run ends (16 divergent call sites)
        uint32_t cur = wm[0];
        int start = 0;
#pragma unroll
        for (int i = 1; i < PK; i++) {
            if (i < v && (wm[i] != cur || (PK > 16 && i - start == 16))) {
                emit(start, i - start, cur);
                cur = wm[i]; start = i;
            }
        }
        emit(start, v - start, cur);
        return;
    }
    // a bit per window that starts a run.  The runs are walked in a loop of their own so that emit()
    // -- the expensive part -- runs once per run of the busiest lane (~6 times) instead of once per
    // window position (16 divergent call sites).
    uint32_t starts = 1u;
#pragma unroll
    for (int i = 1; i < PK; i++) starts |= (uint32_t)(wm[i] != wm[i - 1]) << i;
    const uint32_t vmask = v ? 0xffffffffu >> (32 - v) : 0u;    // (v <= PK: the windows the read has in this segment)
    starts &= vmask;
    if constexpr (PK > 16) {
        // no run longer than 16 windows: `cov` = the windows within 15 of a start at or before them; the lowest window
        // that is not lies exactly 16 after a start and becomes one (bit 0 is set, so whatever is not covered lies in
        // the upper half, and the new start covers all that is left of it)
        uint32_t cov = starts;
        cov |= cov << 1; cov |= cov << 2; cov |= cov << 4; cov |= cov << 8;
        const uint32_t unc = ~cov & vmask;
        starts |= unc & (0u - unc);
    }
    int vend = v;                                      // where the segment's last run ends
    if constexpr (MERGE) {
        const int lane = (int)(threadIdx.x & 63);
        const uint32_t rest = starts & (starts - 1);
        const int b = !v ? 0 : rest ? __ffs((int)rest) - 1 : v;            // head: 1..16 windows, 0 = none
        const int t = v == PK ? __clz((int)starts) + 1 : 0;                // tail of a FULL segment: 1..16 windows, 0 = none
        const uint32_t hk = wm[0], tk = wm[PK - 1];
        // down: the next lane's head key, and its head length below the 13 bases that follow this lane's 64 (a record
        // holds 46 bases from a window <= 31); up: the previous lane's tail
        const uint32_t hk_n = (uint32_t)__shfl_down((int)hk, 1);
        const uint32_t pk_n = (uint32_t)__shfl_down((int)(((uint32_t)(lo >> 32) & 0xFFFFFFC0u) | (uint32_t)b), 1);
        const uint32_t tk_p = (uint32_t)__shfl_up((int)tk, 1);
        const int t_p = __shfl_up(t, 1);
        const bool next_same = lane < 63 && sgm + 1 < s.segs, prev_same = lane > 0 && sgm > 0;   // the same read, the same wave
        const int b_n = (int)(pk_n & 31u);
        if (nx_out) *nx_out = next_same ? pk_n & 0xFFFFFFC0u : 0u;
        if (next_same && t > 0 && b_n > 0 && tk == hk_n) vend = v + (16 - t < b_n ? 16 - t : b_n);
        if (prev_same && t_p > 0 && b > 0 && tk_p == hk) {
            const int a = 16 - t_p < b ? 16 - t_p : b;                     // windows of the head that the tail's owner emits
            if (a > 0) starts = (starts & ~1u) | (a < b ? 1u << a : 0u);
        }
    }
    if (wm_lds) {
#pragma unroll
        for (int i = 0; i < PK; i++) wm_lds[i * SKT + threadIdx.x] = wm[i];
    }
    // (the loop below picks wm[i0] with a tree of selects.  A select between two ELEMENTS of an array is turned into
    // an indexed load by the compiler, and the array into scratch memory: the minima become sixteen scalars, results of
    // an empty asm, which are no elements of anything)
    uint32_t m0 = wm[0], m1 = wm[1], m2 = wm[2], m3 = wm[3], m4 = wm[4], m5 = wm[5], m6 = wm[6], m7 = wm[7], m8 = wm[8],
             m9 = wm[9], m10 = wm[10], m11 = wm[11], m12 = wm[12], m13 = wm[13], m14 = wm[14], m15 = wm[15];
    if (!wm_lds)
        asm("" : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7), "+v"(m8), "+v"(m9), "+v"(m10),
                 "+v"(m11), "+v"(m12), "+v"(m13), "+v"(m14), "+v"(m15));
    constexpr int UP = PK > 16 ? 16 : 0;               // (SEG = 16: the upper sixteen alias the lower and are never selected)
    uint32_t n0 = wm[UP + 0], n1 = wm[UP + 1], n2 = wm[UP + 2], n3 = wm[UP + 3], n4 = wm[UP + 4], n5 = wm[UP + 5], n6 = wm[UP + 6],
             n7 = wm[UP + 7], n8 = wm[UP + 8], n9 = wm[UP + 9], n10 = wm[UP + 10], n11 = wm[UP + 11], n12 = wm[UP + 12],
             n13 = wm[UP + 13], n14 = wm[UP + 14], n15 = wm[UP + 15];
    if (!wm_lds && PK > 16)
        asm("" : "+v"(n0), "+v"(n1), "+v"(n2), "+v"(n3), "+v"(n4), "+v"(n5), "+v"(n6), "+v"(n7), "+v"(n8), "+v"(n9), "+v"(n10),
                 "+v"(n11), "+v"(n12), "+v"(n13), "+v"(n14), "+v"(n15));
    while (starts) {
        const int i0 = __ffs((int)starts) - 1;
        starts &= starts - 1;
        const int i1 = starts ? __ffs((int)starts) - 1 : vend;
        // wm[i0]: a register array cannot be indexed at run time -- through the thread's own LDS column
        // when the caller has one (16 conflict-free stores, one load per run), else a compare-select chain
        uint32_t key;
        if (wm_lds) {
            key = wm_lds[i0 * SKT + threadIdx.x];
        } else {
            // (a tree of selects on the bits of i0: 15 selects under 4 masks, where a chain of 15 compares each waits
            // for its own mask)
            const bool b0 = i0 & 1, b1 = i0 & 2, b2 = i0 & 4, b3 = i0 & 8;
            const uint32_t a0 = b0 ? m1 : m0, a1 = b0 ? m3 : m2, a2 = b0 ? m5 : m4, a3 = b0 ? m7 : m6, a4 = b0 ? m9 : m8,
                           a5 = b0 ? m11 : m10, a6 = b0 ? m13 : m12, a7 = b0 ? m15 : m14;
            const uint32_t c0 = b1 ? a1 : a0, c1 = b1 ? a3 : a2, c2 = b1 ? a5 : a4, c3 = b1 ? a7 : a6;
            const uint32_t d0 = b2 ? c1 : c0, d1 = b2 ? c3 : c2;
            key = b3 ? d1 : d0;
            if constexpr (PK > 16) {                   // a fifth level: the same tree over the upper sixteen
                const uint32_t e0 = b0 ? n1 : n0, e1 = b0 ? n3 : n2, e2 = b0 ? n5 : n4, e3 = b0 ? n7 : n6, e4 = b0 ? n9 : n8,
                               e5 = b0 ? n11 : n10, e6 = b0 ? n13 : n12, e7 = b0 ? n15 : n14;
                const uint32_t f0 = b1 ? e1 : e0, f1 = b1 ? e3 : e2, f2 = b1 ? e5 : e4, f3 = b1 ? e7 : e6;
                const uint32_t g0 = b2 ? f1 : f0, g1 = b2 ? f3 : f2;
                const uint32_t ku = b3 ? g1 : g0;
                key = (i0 & 16) ? ku : key;
            }
        }
        emit(i0, i1 - i0, key);
    }
}

__device__ __forceinline__ uint64_t mmer_hash64(uint32_t canon) { return kmer_hash((uint64_t)canon); }

__device__ __forceinline__ unsigned sk_digit(uint32_t canon, const Level &lv) {
    const uint64_t h = mmer_hash64(canon);
    if (lv.n_owners > 0) {
        const unsigned o = (unsigned)__umul64hi(h, (uint64_t)lv.n_owners);
        return lv.sub_bits ? (o << lv.sub_bits) | ((uint32_t)((h << OWNER_BITS) >> 32) >> (32 - lv.sub_bits)) : o;
    }
    return rec_digit((uint32_t)((h << OWNER_BITS) >> 32), 0, lv.bits);
}

// Run descriptors: what the scatter needs to know about a segment without redoing the minimiser
// arithmetic (two thirds of both kernels' instructions).  desc[g] = run-start bits of segment g |
// runs << 16, desc[(1 + r) * n_threads + g] = header word (32 hash bits) of its r-th run, r < SKD.
// Word-major, so the lanes of a wave store / load consecutive words; a segment with more than SKD
// runs (0.02 %) makes its wave recompute.
constexpr int SKD = 8;

// WIDE: a k = 33..63 source (read_nk)
template <int W, bool DESC, bool WIDE = false>
__global__ __launch_bounds__(SKT) void k_sk_hist(ReadSrc s, Level lv, uint64_t *__restrict__ blockhist,
                                                 uint32_t *__restrict__ desc) {
    __shared__ uint32_t h[1 << MAX_BITS];
    __shared__ uint32_t wmcol[DESC ? PK * SKT : 1];      // per-window minimisers, one column per thread
    const int nb = lv.n_owners > 0 ? lv.n_owners : (1 << lv.bits);
    for (int i = threadIdx.x; i < nb; i += SKT) h[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * SKT;
    const int64_t dq = stride / s.segs;
    const int dr = (int)(stride - dq * s.segs);
    int64_t g = (int64_t)blockIdx.x * SKT + threadIdx.x;
    SegPos q;
    q.r = g / s.segs;
    q.sgm = (int)(g - q.r * s.segs);
    for (; g < s.n_threads; g += stride) {
        uint64_t w[3], hi, lo;
        seg_load(s, q, w);
        if constexpr (DESC) {
            uint32_t mask = 0, nr = 0;
            // run loop: the r-th run of every lane is handled in the same iteration, so the header
            // stores of a wave go to consecutive words
            uint32_t own[2] = {0, 0};                    // owner mode: the runs' owners, 8 bits each
            seg_runs<W, true>(s, read_nk<WIDE>(s, q.r), q.sgm, w, [&](int i0, int, uint32_t canon) {
                const uint64_t h64 = mmer_hash64(canon);
                const uint32_t hdr = (uint32_t)((h64 << OWNER_BITS) >> 32);
                const unsigned d = lv.n_owners > 0 ? (unsigned)__umul64hi(h64, (uint64_t)lv.n_owners) : rec_digit(hdr, 0, lv.bits);
                atomicAdd(&h[d], 1u);
                if (nr < (uint32_t)SKD) {
                    desc[(int64_t)(1 + nr) * s.n_threads + g] = hdr;
                    if (nr < 4) own[0] |= d << (8 * nr); else own[1] |= d << (8 * (nr - 4));
                }
                mask |= 1u << i0; nr++;
            }, &hi, &lo, wmcol);
            desc[g] = mask | (nr << 16);
            if (lv.n_owners > 0) {
                desc[(int64_t)(1 + SKD) * s.n_threads + g] = own[0];
                desc[(int64_t)(2 + SKD) * s.n_threads + g] = own[1];
            }
        } else {
            seg_runs<W, false>(s, read_nk<WIDE>(s, q.r), q.sgm, w, [&](int, int, uint32_t canon) { atomicAdd(&h[sk_digit(canon, lv)], 1u); }, &hi, &lo);
        }
        q.r += dq; q.sgm += dr;
        if (q.sgm >= s.segs) { q.sgm -= s.segs; q.r++; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += SKT) blockhist[(int64_t)i * gridDim.x + blockIdx.x] = h[i];
}

// Records leave through write-combining rings (see k_rec_scatter_wc): every private per-digit
// stream has SKB record slots in LDS indexed by the record's final position, and only whole
// aligned 64-byte lines are stored; a digit that overruns its ring in one round stores directly.
constexpr int SKB = 8, SKA = 4;
// WIDE: the 32-byte records of the k = 33..63 path (s.k = the central window, s.wfl = the flank)
template <int W, bool DESC, bool WIDE = false>
__global__ __launch_bounds__(SKT, WIDE ? 4 : 8) void k_sk_scatter(ReadSrc s, Level lv, const uint64_t *__restrict__ scanned,
                                                              std::conditional_t<WIDE, WRec, Rec> *__restrict__ out,
                                                              const uint32_t *__restrict__ desc) {
    using RT = std::conditional_t<WIDE, WRec, Rec>;
    extern __shared__ __attribute__((aligned(32))) unsigned char sk_smem[];
    const int nb = lv.n_owners > 0 ? lv.n_owners : (1 << lv.bits);
    // (the rings are addressed through these expressions, not through pointer variables: a pointer
    // captured by the lambdas below decays to a generic one and the LDS atomics with it)
#define buf ((RT *)sk_smem)
#define tail ((unsigned long long *)(sk_smem + (size_t)nb * SKB * sizeof(RT)))
#define head (tail + nb)
    for (int i = threadIdx.x; i < nb; i += SKT) tail[i] = head[i] = scanned[(int64_t)i * gridDim.x + blockIdx.x];
    __syncthreads();
    auto drain = [&](bool final) __attribute__((always_inline)) {
        for (int d = threadIdx.x / SKB; d < nb; d += SKT / SKB) {
            const int j = threadIdx.x % SKB;
            const unsigned long long h = head[d], t = tail[d];
            unsigned long long e, nh;
            if (t - h > (unsigned long long)SKB) { e = h + SKB; nh = t; }     // the excess went out directly
            else {
                e = final ? t : (t & ~(unsigned long long)(SKA - 1));
                if (e < h) e = h;
                nh = e;
            }
            const unsigned long long g = h + j;
            if (g < e) out[g] = buf[(size_t)d * SKB + (g & (SKB - 1))];
            if (j == 0) head[d] = nh;
        }
    };
    const int64_t stride = (int64_t)gridDim.x * SKT;
    const int64_t dq = stride / s.segs;
    const int dr = (int)(stride - dq * s.segs);
    const int64_t g0 = (int64_t)blockIdx.x * SKT;
    int64_t g = g0 + threadIdx.x;
    SegPos q;
    q.r = g / s.segs;
    q.sgm = (int)(g - q.r * s.segs);
    // every thread of the workgroup runs the same number of rounds (the barriers are uniform)
    for (int64_t gb = g0; gb < s.n_threads; gb += stride, g += stride) {
        if (g < s.n_threads) {
            uint64_t w[3], hi = 0, lo = 0;
            seg_load(s, q, w);
            // one record: windows [i0, i0 + n) of the segment, header word hdr, digit d
            auto put = [&](int i0, int n, uint32_t hdr, unsigned d) __attribute__((always_inline)) {
                RT r;
                if constexpr (WIDE) {
                    // 96 bases from the first base of the run's first k-mer: the central window starts
                    // s.wfl bases further on (words past the read's end are never used: k + n - 1 bases are)
                    const uint64_t *gw = s.words + q.r * s.wpr;
                    const int p = s.fc - s.wfl + q.sgm * PK + i0;
                    const int wi = p >> 5, sft = 2 * (p & 31), last = s.wpr - 1;
                    const uint64_t a0 = gw[wi < last ? wi : last], a1 = gw[wi + 1 < last ? wi + 1 : last];
                    const uint64_t a2 = gw[wi + 2 < last ? wi + 2 : last], a3 = gw[wi + 3 < last ? wi + 3 : last];
                    r.b0 = sft ? (a0 << sft) | (a1 >> (64 - sft)) : a0;
                    r.b1 = sft ? (a1 << sft) | (a2 >> (64 - sft)) : a1;
                    r.b2 = sft ? (a2 << sft) | (a3 >> (64 - sft)) : a2;
                    r.hd = ((uint64_t)(n - 1) << 32) | (uint64_t)hdr;
                } else {
                    const int sft = 2 * i0;
                    r.w0 = sft ? (hi << sft) | (lo >> (64 - sft)) : hi;
                    r.w1 = ((lo << sft) & 0xFFFFFFF000000000ULL) | ((uint64_t)(n - 1) << 32) | (uint64_t)hdr;
                }
                const unsigned long long pos = atomicAdd(&tail[d], 1ULL);
                if (pos - head[d] < (unsigned long long)SKB) buf[(size_t)d * SKB + (pos & (SKB - 1))] = r;
                else out[pos] = r;
            };
            // `hi`/`lo` are written before the first emit() runs (seg_runs stores them first)
            auto recompute = [&]() __attribute__((always_inline)) {
                seg_runs<W, true>(s, read_nk<WIDE>(s, q.r), q.sgm, w, [&](int i0, int n, uint32_t canon) {
                    const uint64_t h = mmer_hash64(canon);
                    const unsigned d = lv.n_owners > 0 ? (unsigned)__umul64hi(h, (uint64_t)lv.n_owners)
                                                       : rec_digit((uint32_t)((h << OWNER_BITS) >> 32), 0, lv.bits);
                    put(i0, n, (uint32_t)((h << OWNER_BITS) >> 32), d);
                }, &hi, &lo);
            };
            if constexpr (DESC) {
                const uint32_t m = desc[g];
                const uint32_t nr = m >> 16;
                if (nr > (uint32_t)SKD) {
                    recompute();
                } else if (nr) {
                    // the 64 bases from the segment's first window on (as seg_runs forms them)
                    const int p0 = q.sgm * PK;
                    int v = read_nk<WIDE>(s, q.r) - p0;
                    v = v > PK ? PK : v;
                    const int sh = 2 * ((s.fc + p0) & 31);
                    hi = sh ? (w[0] << sh) | (w[1] >> (64 - sh)) : w[0];
                    lo = sh ? (w[1] << sh) | (w[2] >> (64 - sh)) : w[1];
                    // all header words of the segment at once: SKD independent loads in flight instead of
                    // one exposed memory latency per run
                    uint32_t hd[SKD];
#pragma unroll
                    for (int r = 0; r < SKD; r++) hd[r] = (uint32_t)r < nr ? desc[(int64_t)(1 + r) * s.n_threads + g] : 0u;
                    uint32_t own[2] = {0, 0};
                    if (lv.n_owners > 0) {
                        own[0] = desc[(int64_t)(1 + SKD) * s.n_threads + g];
                        own[1] = desc[(int64_t)(2 + SKD) * s.n_threads + g];
                    }
                    uint32_t starts = m & 0xffffu;
#pragma unroll
                    for (int r = 0; r < SKD; r++) {
                        if (starts) {
                            const int i0 = __ffs((int)starts) - 1;
                            starts &= starts - 1;
                            const int i1 = starts ? __ffs((int)starts) - 1 : v;
                            put(i0, i1 - i0, hd[r], lv.n_owners > 0 ? (own[r >> 2] >> (8 * (r & 3))) & 255u : rec_digit(hd[r], 0, lv.bits));
                        }
                    }
                }
            } else {
                recompute();
            }
            q.r += dq; q.sgm += dr;
            if (q.sgm >= s.segs) { q.sgm -= s.segs; q.r++; }
        }
        __syncthreads();
        drain(false);
        __syncthreads();
    }
    drain(true);
}
#undef buf
#undef tail
#undef head

// ---- level 1 in ONE sweep over the reads.  The two-pass form above computes every minimiser in the histogram pass
// and carries 5.4 GB of run descriptors to the scatter so as not to compute them twice.  Here nothing is counted first:
// a sampled histogram (one tile of 1024 segments in every `sample`) sizes a REGION per bucket with room to spare, and a
// workgroup takes its output positions from the bucket's cursor in EXTENTS of OSE records (one global atomic per
// extent).  A workgroup always owns the extent it is filling and the next one, so the write-combining rings and the
// direct stores of a busy round never wait for an allocation; extents change hands only at the round's barrier.
// What a workgroup leaves unused of its last two extents are HOLES; k_fix_holes moves the records at the end of every
// bucket into the holes before it, so the next level reads a gap-free [seg_begin, seg_end) per bucket.  A region that
// runs out (a sample that missed the skew) raises `overflow` and the caller falls back to the two-pass form.
constexpr int OSE_MIN = 64, OSE_MAX = 256;   // records per extent: a round must not put more than one extent of one
                                         // workgroup into one bucket (5 records on average at 512 buckets); the sampled
                                         // histogram picks 64, 128 or 256 by the busiest bucket, or no sweep at all
constexpr int OS_CSTRIDE = 16;           // cursors 128 bytes apart: one atomic unit each
constexpr int OS_MAXG = 512;             // workgroups of the sweep
constexpr int OS_HOLES = 3;              // extents a workgroup has in hand per bucket: filling, next, requested
struct OneSweep {
    const uint64_t *reg_start;           // [nb + 1] first record of every region (multiples of the extent); [nb] = a dump extent
    const uint32_t *reg_cap;             // [nb] records a region holds
    unsigned long long *cursor;          // [nb * OS_CSTRIDE] next record to hand out (absolute; starts at reg_start)
    uint64_t *holes;                     // [nb][OS_HOLES * G] (absolute start << 16) | length, 0 = none
    int *overflow;                       // [0] the sweep is void (1; 2: k_fix_holes' books do not balance), [1] a round raised it
    uint64_t total;                      // records allocated (regions + the dump extent)
    unsigned long long *tile_counter;    // tiles of SKT segments handed out beyond every workgroup's first two
    uint32_t ose, ose_shift;             // records per extent (a power of two)
};

template <int W, int SEG = 16, bool WIDE = false>
__global__ __launch_bounds__(SKT) void k_sk_sample_hist(ReadSrc s, Level lv, int sample, unsigned long long *__restrict__ hist) {
    __shared__ uint32_t h[1 << MAX_BITS];
    const int nb = 1 << lv.bits;
    for (int i = threadIdx.x; i < nb; i += SKT) h[i] = 0;
    __syncthreads();
    const int64_t ntile = (s.n_threads + SKT - 1) / SKT;
    for (int64_t T = (int64_t)blockIdx.x * sample; T < ntile; T += (int64_t)gridDim.x * sample) {
        // (32 windows per thread: the runs the sweep will cut, merged across segment edges -- every lane calls seg_runs)
        const int64_t g = T * SKT + threadIdx.x;
        const bool in = g < s.n_threads;
        SegPos q{0, 0};
        int nk_r = 0;
        uint64_t w[3] = {0, 0, 0}, hi, lo;
        if (in) {
            q.r = g / s.segs;
            q.sgm = (int)(g - q.r * s.segs);
            seg_load<SEG>(s, q, w);
            nk_r = read_nk<WIDE>(s, q.r);
        }
        if (SEG == 32 || in)
            seg_runs<W, SEG == 32, SEG>(s, nk_r, q.sgm, w, [&](int, int, uint32_t canon) { atomicAdd(&h[sk_digit(canon, lv)], 1u); }, &hi, &lo);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += SKT) if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// regions from the sampled histogram: estimate + six standard deviations of the sample + 1/64 + what the workgroups
// hold in hand; totals[0] = records to allocate (regions + the dump extent), totals[2] = records per extent: four times
// what a tile is expected to put into the busiest bucket, or 0 = no sweep (low-complexity reads on one minimiser)
__global__ __launch_bounds__(1024) void k_plan_regions(const unsigned long long *__restrict__ hist, int nb, double scale, int G, int cap_pct,
                                                       double tiles,
                                                       uint64_t *__restrict__ reg_start, uint32_t *__restrict__ reg_cap,
                                                       unsigned long long *__restrict__ cursor, unsigned long long *__restrict__ totals) {
    __shared__ uint64_t caps[1 << MAX_BITS];
    __shared__ unsigned long long busiest;
    __shared__ uint32_t ose_s;
    const int d = threadIdx.x;
    if (d == 0) busiest = 0;
    __syncthreads();
    if (d < nb) atomicMax(&busiest, hist[d]);
    __syncthreads();
    if (d == 0) {
        const double per_tile = (double)busiest * scale / tiles;       // records a tile puts into the busiest bucket
        ose_s = per_tile <= 16.0 ? 64u : per_tile <= 32.0 ? 128u : per_tile <= 64.0 ? 256u : 0u;
    }
    __syncthreads();
    const uint32_t E = ose_s ? ose_s : OSE_MIN;
    if (d < nb) {
        const double c = (double)hist[d];
        const double est = c * scale;
        double room = (est + 6.0 * scale * sqrt(c + 1.0) + est / 64.0 + 1024.0) * (double)cap_pct / 100.0;
        uint64_t cap = (uint64_t)room + (uint64_t)G * OS_HOLES * E;
        cap = (cap + E - 1) / E * E;
        if (cap > 0xFFFFFF00ULL) cap = 0xFFFFFF00ULL / E * E;          // bucket-local positions are 32-bit
        caps[d] = cap;
        reg_cap[d] = (uint32_t)cap;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t at = 0;
        for (int i = 0; i < nb; i++) { reg_start[i] = at; cursor[(size_t)i * OS_CSTRIDE] = at; at += caps[i]; }
        reg_start[nb] = at;
        totals[0] = at + E;
        totals[1] = 0;
        totals[2] = ose_s;
    }
}

// WIDE: the 32-byte records of the k = 33..63 path (as in k_sk_scatter)
// SEG: windows a thread owns (seg_runs).  32: one workgroup per CU (the minima of 32 windows and 50 m-mers live in
// registers) with rings of OSB = 16 records, since a round now brings a bucket 8 records on average.
// (first form: 1024 threads, one workgroup per CU, rings of 16: no faster than 16 windows per thread -- the instructions
// saved went into the CU standing still at the round's two barriers.  Hence T = 512 threads: two workgroups per CU again,
// a tile brings a bucket what it did before, and the rings stay at 8 slots.)
template <int SEG, bool WIDE> struct OsGeo {
    static constexpr int T = SEG > 16 && !WIDE ? 512 : SKT;                  // threads per workgroup = segments per tile
};
// (four waves per SIMD in every form: the rings of 512 buckets let two workgroups of 512 threads share a CU, those of
// 1024 buckets -- the only case that runs the 16-window form of the 16-byte records -- and of the 32-byte records one of 1024)
template <int W, bool WIDE = false, int SEG = 16>
__global__ __launch_bounds__((OsGeo<SEG, WIDE>::T), 4) void k_sk_onesweep(ReadSrc s, Level lv, OneSweep os,
                                                               std::conditional_t<WIDE, WRec, Rec> *__restrict__ out) {
    using RT = std::conditional_t<WIDE, WRec, Rec>;
    constexpr int SKT = OsGeo<SEG, WIDE>::T;                                  // (shadows the file-wide workgroup size)
    extern __shared__ __attribute__((aligned(32))) unsigned char sk_smem[];
    const int nb = 1 << lv.bits;
#define buf ((RT *)sk_smem)
#define tail ((uint32_t *)(sk_smem + (size_t)nb * SKB * sizeof(RT)))        /* records given a (workgroup-local) position */
#define head (tail + nb)                                                    /* ... of them stored */
#define cstart (tail + 2 * nb)                                              /* local position the current extent starts at */
#define cbase (tail + 3 * nb)                                               /* the current extent (its number: record / OSE) */
#define nbase (tail + 4 * nb)                                               /* the next one */
#define pbase (tail + 5 * nb)                                               /* the one after that, or NONE while it is on order */
    constexpr uint32_t DUMP = 0xFFFFFFFFu;
    const uint32_t OSE = os.ose, OSH = os.ose_shift;
    const uint64_t dump_at = os.total - OSE;
    // An extent off bucket d's cursor.  Only the END OF THE ALLOCATION is checked here (no load on this path): an extent
    // past the bucket's own region lands in its neighbour's, which k_fix_holes sees from the cursor and declares the
    // whole sweep void.
    auto extent_of = [&](unsigned long long b) __attribute__((always_inline)) -> uint32_t {
        return b + OSE <= dump_at ? (uint32_t)(b >> OSH) : DUMP;
    };
    auto grab = [&](int d) __attribute__((always_inline)) -> uint32_t {
        return extent_of(atomicAdd(&os.cursor[(size_t)d * OS_CSTRIDE], (unsigned long long)OSE));
    };
    // where local position v of a bucket lives (v - cs < 2 * OSE)
    auto phys = [&](uint32_t v, uint32_t cs, uint32_t cb, uint32_t nx) __attribute__((always_inline)) -> uint64_t {
        const uint32_t o = v - cs;
        const uint32_t b = o < (uint32_t)OSE ? cb : nx;
        return (b == DUMP ? dump_at : (uint64_t)b << OSH) + (o & (OSE - 1));
    };
    // The extent after the next one is requested a round ahead: thread d asks for bucket d's at the top of a round and
    // files it (pbase) at the end of the round's arithmetic, so the atomic has the whole round to come back -- waited
    // for inside the drain it would hold up the wave's stores behind it, round after round.
    constexpr uint32_t NONE = 0xFFFFFFFEu;
    for (int i = threadIdx.x; i < nb; i += SKT) {
        tail[i] = 0; head[i] = 0; cstart[i] = 0;
        cbase[i] = grab(i);
        nbase[i] = grab(i);
        pbase[i] = grab(i);
    }
    __syncthreads();
    // LPB lanes drain a bin, each every LPB-th record of what waits: eight lanes (one record each) in rounds 1-2; four
    // with 32 windows per thread -- a bin's bookkeeping is done by half as many lanes, and four lanes are one aligned
    // 64-byte line, the unit the rings hand out anyway -- and four for the 32-byte records of k = 33..63 (eight: part1
    // 9.95 instead of 9.80 ms)
    constexpr int LPB = SEG > 16 || WIDE ? 4 : SKB;
    auto drain = [&](bool final) __attribute__((always_inline)) {
#pragma nounroll
        for (int d = threadIdx.x / LPB; d < nb; d += SKT / LPB) {
            const int j = threadIdx.x % LPB;
            const uint32_t h = head[d], t = tail[d], cs = cstart[d], cb = cbase[d], nx = nbase[d];
            uint32_t e, nh;
            if (t - h > (uint32_t)SKB) { e = h + SKB; nh = t; }               // the excess went out directly
            else {
                e = final ? t : (t & ~(uint32_t)(SKA - 1));
                if (e < h) e = h;
                nh = e;
            }
#pragma unroll
            for (int q = 0; q < SKB / LPB; q++) {
                const uint32_t g = h + j + q * LPB;
                if (g < e) l2_store_stream(out + phys(g, cs, cb, nx), buf[(size_t)d * SKB + (g & (SKB - 1))]);
            }
            if (j == 0) {
                head[d] = nh;
                // The extent that lies wholly behind the stored position is done with: move up ONE extent (the lanes of
                // this bucket read the old values above, in lock-step).  No claim here: a returning atomic in this loop
                // puts an s_waitcnt vmcnt(0) on its back edge, and every iteration then waits for its own stores.
                // One step is enough.  The emit takes positions below cstart + 2 OSE only, so nh - cs <= 2 OSE while
                // the flag is down, and after the step nh - cstart <= OSE.  At equality the current extent is exactly
                // full and nothing lies in the next one: the coming round has one extent of room where it has two
                // otherwise, the step after it is due at the next drain, and `used == OSE` leaves no hole below.
                // pbase[d] is valid here: it is refilled at the top of every round that finds it NONE.  Only the last
                // drain can find NONE (the drain before it took the extent): nothing is stored after it, so the
                // bucket goes on without a next extent (DUMP: no hole).
                // With the flag up, tail runs ahead of what was stored and the bookkeeping may be anything; phys()
                // still returns (cbase or nbase or the dump extent) + (offset & (OSE - 1)), and neither cbase nor
                // nbase is ever NONE, so every store lands in an extent this workgroup claimed or in the dump extent.
                if (nh - cs >= (uint32_t)OSE) {
                    const uint32_t b2 = pbase[d];
                    cstart[d] = cs + OSE; cbase[d] = nx; nbase[d] = final && b2 == NONE ? DUMP : b2; pbase[d] = NONE;
                }
            }
        }
    };
    // Tiles of SKT segments are handed out by a global counter (a workgroup's first two are its number and its number
    // + gridDim.x): the workgroups stay as few as the holes allow and still finish together.  The tile after the next is
    // asked for at the top of a round, like the extents: the next one is then known, and its words travel during the round.
    __shared__ long long tile_lds[2];
    const int64_t ntile = (s.n_threads + SKT - 1) / SKT;
    const int my_d = (int)threadIdx.x;                  // the bucket this thread keeps supplied (nb <= SKT)
    int64_t T = blockIdx.x;
    // where the thread's segment of a tile lies, and its words on their way (no branch, so no wait of its own: a lane
    // past the last segment, or a tile past the last, reads the last segment's words, and `in` drops them)
    auto fetch = [&](int64_t tile, SegPos &q, int &nk_r, uint64_t (&w)[3]) __attribute__((always_inline)) {
        const int64_t g = tile * SKT + threadIdx.x;
        const int64_t gc = g < s.n_threads ? g : s.n_threads - 1;
        q.r = gc / s.segs;
        q.sgm = (int)(gc - q.r * s.segs);
        seg_load<SEG>(s, q, w);
        nk_r = read_nk<WIDE>(s, q.r);
    };
    int64_t T1 = (int64_t)gridDim.x + blockIdx.x;      // the tile after this one (the counter hands out from 2 gridDim.x)
    SegPos qn{0, 0};
    int nkn = 0;
    uint64_t wn[3] = {0, 0, 0};
    if (T < ntile) fetch(T, qn, nkn, wn);
    asm volatile("" : "+v"(wn[0]), "+v"(wn[1]), "+v"(wn[2]), "+v"(nkn));
    for (int rnd = 0; T < ntile; rnd++) {
        // A round waits for memory ONCE, after its arithmetic.  The words of this round's tile were requested a round
        // ago; the next tile's (known a round ahead: the counter is asked for the tile after the next) are requested here
        // with the extent claim and the tile claim, and every lane awaits all of it after seg_runs, before the drain --
        // whatever branch it takes, so that nothing but stores is in flight at the drain and at the next round's top (a
        // result that some path never uses counts as in flight there, and the wait the compiler then puts is a vmcnt(0)
        // that also waits for the drain's stores).
        // (SEG = 32: every lane calls seg_runs, which swaps run ends with the neighbour lanes; a lane past the last
        // segment brings no windows)
        const bool in = T * SKT + threadIdx.x < s.n_threads;
        SegPos q{in ? qn.r : 0, in ? qn.sgm : 0};
        int nk_r = in ? nkn : 0;
        uint64_t w[3] = {in ? wn[0] : 0, in ? wn[1] : 0, in ? wn[2] : 0}, hi = 0, lo = 0;
        uint32_t past = 0;                              // the 13 bases after (hi, lo), from the next lane (SEG = 32)
        unsigned long long t_raw = 0, req_raw = 0;
        const bool ask = my_d < nb && pbase[my_d] == NONE;
        if (ask) req_raw = atomicAdd(&os.cursor[(size_t)my_d * OS_CSTRIDE], (unsigned long long)OSE);
        fetch(T1, qn, nkn, wn);
        if (threadIdx.x == SKT - 1) t_raw = atomicAdd(os.tile_counter, 1ULL);
        if (SEG == 32 || in) {
            seg_runs<W, true, SEG>(s, nk_r, q.sgm, w, [&](int i0, int n, uint32_t canon) {
                const uint64_t hh = mmer_hash64(canon);
                const uint32_t hdr = (uint32_t)((hh << OWNER_BITS) >> 32);
                // (by owner: the owner's bucket is 2^sub_bits bins here, so that a round still brings a bin a handful of
                // records -- the receiver does not care which of them a record came through)
                const unsigned d = lv.n_owners > 0 ? (((unsigned)__umul64hi(hh, (uint64_t)lv.n_owners) << lv.sub_bits) | (hdr >> (32 - lv.sub_bits)))
                                                   : rec_digit(hdr, 0, lv.bits);
                RT r;
                if constexpr (WIDE) {
                    // 96 bases from the first base of the run's first k-mer (see k_sk_scatter)
                    const uint64_t *gw = s.words + q.r * s.wpr;
                    const int p = s.fc - s.wfl + q.sgm * SEG + i0;
                    const int wi = p >> 5, sft = 2 * (p & 31), last = s.wpr - 1;
                    const uint64_t a0 = gw[wi < last ? wi : last], a1 = gw[wi + 1 < last ? wi + 1 : last];
                    const uint64_t a2 = gw[wi + 2 < last ? wi + 2 : last], a3 = gw[wi + 3 < last ? wi + 3 : last];
                    r.b0 = sft ? (a0 << sft) | (a1 >> (64 - sft)) : a0;
                    r.b1 = sft ? (a1 << sft) | (a2 >> (64 - sft)) : a1;
                    r.b2 = sft ? (a2 << sft) | (a3 >> (64 - sft)) : a2;
                    r.hd = ((uint64_t)(n - 1) << 32) | (uint64_t)hdr;
                } else {
                    // (a run that starts after window 18 reaches into the next lane's bases -- a merged tail needs them)
                    // 92 bits from bit 2 i0 of the 160-bit string (hi, lo, past), by 32-bit funnel shifts: the string
                    // shifted right by one bit (e0..e4, the same for every run of the thread) makes the shift 31 - t with
                    // t = 2 (i0 & 15), in 1..31 -- v_alignbit_b32 takes no shift of 32 -- and i0 >> 4 picks the first word
                    const uint32_t d0 = (uint32_t)(hi >> 32), d1 = (uint32_t)hi, d2 = (uint32_t)(lo >> 32), d3 = (uint32_t)lo;
                    const uint32_t e0 = d0 >> 1, e1 = __builtin_amdgcn_alignbit(d0, d1, 1), e2 = __builtin_amdgcn_alignbit(d1, d2, 1);
                    const uint32_t e3 = __builtin_amdgcn_alignbit(d2, d3, 1), e4 = __builtin_amdgcn_alignbit(d3, past, 1);
                    const bool up = i0 >= 16;
                    const uint32_t a0 = up ? e1 : e0, a1 = up ? e2 : e1, a2 = up ? e3 : e2, a3 = up ? e4 : e3;
                    const uint32_t sh = 31u - 2u * ((uint32_t)i0 & 15u);
                    const uint32_t w0h = __builtin_amdgcn_alignbit(a0, a1, sh), w0l = __builtin_amdgcn_alignbit(a1, a2, sh);
                    const uint32_t w1h = (__builtin_amdgcn_alignbit(a2, a3, sh) & 0xFFFFFFF0u) | (uint32_t)(n - 1);
                    r.w0 = ((uint64_t)w0h << 32) | w0l;
                    r.w1 = ((uint64_t)w1h << 32) | (uint64_t)hdr;
                }
                const uint32_t pos = atomicAdd(&tail[d], 1u);
                if (pos - head[d] < (uint32_t)SKB) buf[(size_t)d * SKB + (pos & (SKB - 1))] = r;
                else {
                    const uint32_t cs = cstart[d];
                    if (pos - cs < 2u * OSE) out[phys(pos, cs, cbase[d], nbase[d])] = r;
                    else { os.overflow[0] = 1; os.overflow[1] = 1; }   // more than the two extents in hand take: the caller starts over
                }
            }, &hi, &lo, nullptr, &past);
        }
        asm volatile("" : "+v"(wn[0]), "+v"(wn[1]), "+v"(wn[2]), "+v"(nkn), "+v"(t_raw), "+v"(req_raw));
        if (threadIdx.x == SKT - 1) tile_lds[rnd & 1] = 2LL * (long long)gridDim.x + (long long)t_raw;
        if (ask) pbase[my_d] = extent_of(req_raw);
        __syncthreads();
        drain(false);
        T = T1;
        T1 = tile_lds[rnd & 1];
        __syncthreads();
    }
    drain(true);
    __syncthreads();
    // what is left of the extents in hand (after the last drain: head == tail, tail - cstart <= OSE)
    for (int d = threadIdx.x; d < nb; d += SKT) {
        const uint32_t used = tail[d] - cstart[d], cb = cbase[d], nx = nbase[d], px = pbase[d];
        uint64_t *hl = os.holes + ((size_t)d * gridDim.x + blockIdx.x) * OS_HOLES;
        hl[0] = cb != DUMP && used < OSE ? ((((uint64_t)cb << OSH) + used) << 16) | (uint64_t)(OSE - used) : 0;
        hl[1] = nx != DUMP ? (((uint64_t)nx << OSH) << 16) | (uint64_t)OSE : 0;
        hl[2] = px != DUMP && px != NONE ? (((uint64_t)px << OSH) << 16) | (uint64_t)OSE : 0;
    }
}
#undef buf
#undef tail
#undef head
#undef cstart
#undef cbase
#undef nbase
#undef pbase

// One workgroup per bucket: the bucket's cursor says how far extents were handed out (alloc), the holes sum to H, so
// the bucket holds size = alloc - H records and the last H positions [size, alloc) -- the tail zone -- hold as many
// records as there are hole positions before `size`.  Tail record i goes to hole position i.
constexpr int FH_T = 1024;
template <class RT>
__global__ __launch_bounds__(FH_T) void k_fix_holes(OneSweep os, int G, RT *__restrict__ out, uint64_t *__restrict__ seg_begin,
                                                   uint64_t *__restrict__ seg_end, unsigned long long *__restrict__ totals) {
    constexpr int NHMAX = 2048;                                // holes of a bucket (>= OS_HOLES * OS_MAXG, a multiple of FH_T)
    static_assert(NHMAX >= OS_HOLES * OS_MAXG && NHMAX % FH_T == 0, "holes per bucket");
    constexpr int NWMAX = NHMAX * OSE_MAX / 32;                // words of the tail-zone bitmap
    __shared__ uint32_t hstart[NHMAX], hoff[NHMAX + 1];
    __shared__ uint32_t bitmap[NWMAX];
    __shared__ uint32_t wsum[FH_T / 64];
    const int d = blockIdx.x;
    const int NH = OS_HOLES * G;
    const uint64_t base = os.reg_start[d];
    const unsigned long long alloc = os.cursor[(size_t)d * OS_CSTRIDE] - base;
    if (alloc > (unsigned long long)os.reg_cap[d]) {           // ran over its region: the sweep is void
        if (threadIdx.x == 0) { seg_begin[d] = base; seg_end[d] = base; *os.overflow = 1; }
        return;
    }
    auto block_excl_scan = [&](uint32_t v, uint32_t *total) __attribute__((always_inline)) -> uint32_t {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        uint32_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t b = 0, tot = 0;
        for (int i = 0; i < FH_T / 64; i++) { const uint32_t sv = wsum[i]; if (i < wave) b += sv; tot += sv; }
        __syncthreads();
        *total = tot;
        return b + x - v;
    };
    constexpr int HPT = NHMAX / FH_T;
    uint32_t hs[HPT], hl[HPT];
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < HPT; r++) {
        const int t = threadIdx.x * HPT + r;
        const uint64_t x = t < NH ? os.holes[(size_t)d * NH + t] : 0;
        hl[r] = (uint32_t)(x & 0xFFFFu);
        hs[r] = hl[r] ? (uint32_t)((x >> 16) - base) : 0u;
        mine += hl[r];
    }
    uint32_t H;
    block_excl_scan(mine, &H);
    const uint32_t size = (uint32_t)alloc - H;
    const uint32_t nw = (H + 31) / 32;                         // words of the tail zone's bitmap (<= NWMAX)
    const uint32_t wpt = (nw + FH_T - 1) / FH_T;               // ... a thread looks after: [tid * wpt, tid * wpt + wpt)
    for (uint32_t i = threadIdx.x; i < nw; i += FH_T) bitmap[i] = 0;
    __syncthreads();
    // hole positions before `size` (to be filled) / inside the tail zone (marked)
    uint32_t fill[HPT], fsum = 0;
#pragma unroll
    for (int r = 0; r < HPT; r++) {
        fill[r] = hs[r] < size ? (hs[r] + hl[r] <= size ? hl[r] : size - hs[r]) : 0u;
        fsum += fill[r];
        for (uint32_t p = hs[r] + fill[r]; p < hs[r] + hl[r]; p++) atomicOr(&bitmap[(p - size) >> 5], 1u << ((p - size) & 31));
    }
    uint32_t F;
    uint32_t fo = block_excl_scan(fsum, &F);
#pragma unroll
    for (int r = 0; r < HPT; r++) {
        const int t = threadIdx.x * HPT + r;
        hstart[t] = hs[r]; hoff[t] = fo; fo += fill[r];
    }
    if (threadIdx.x == 0) hoff[NHMAX] = F;
    __syncthreads();
    // records of the tail zone, in position order
    auto valid_word = [&](uint32_t w) __attribute__((always_inline)) -> uint32_t {
        if (w >= nw) return 0u;
        const uint32_t lim = H - w * 32 >= 32 ? 0xFFFFFFFFu : (1u << (H - w * 32)) - 1u;
        return ~bitmap[w] & lim;
    };
    uint32_t vsum = 0;
    for (uint32_t r = 0; r < wpt; r++) vsum += (uint32_t)__popc(valid_word(threadIdx.x * wpt + r));
    uint32_t V;
    uint32_t vo = block_excl_scan(vsum, &V);
    for (uint32_t r = 0; r < wpt; r++) {
        const uint32_t w = threadIdx.x * wpt + r;
        uint32_t m = valid_word(w);
        while (m) {
            const int b = __ffs((int)m) - 1;
            m &= m - 1;
            const uint32_t i = vo++;                           // i-th record of the tail zone -> i-th hole position
            if (i < F) {
                int lo = 0, hi = NHMAX;                        // the entry with hoff <= i < hoff of the next
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (hoff[mid] <= i) lo = mid; else hi = mid; }
                out[base + hstart[lo] + (i - hoff[lo])] = out[base + size + w * 32 + b];
            }
        }
    }
    if (threadIdx.x == 0) {
        seg_begin[d] = base; seg_end[d] = base + size;
        atomicAdd(&totals[1], (unsigned long long)size);
        if (V != F) *os.overflow = 2;                          // cannot happen: the books of the sweep do not balance
    }
}

}  // namespace

namespace rfx {

#define RFX_SK_W_CASES(X) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18)
template <bool DESC, bool WIDE = false, class... Args>
static int launch_sk_hist(rfx_ctx *ctx, int W, dim3 grid, Args... args) {
    if constexpr (WIDE) {                  // the central window is 30 or 31 bases: W = 18 or 19
        if (W == 18) RFX_LAUNCH((k_sk_hist<18, DESC, true>), grid, dim3(SKT), 0, args...);
        else RFX_LAUNCH((k_sk_hist<19, DESC, true>), grid, dim3(SKT), 0, args...);
        return RFX_OK;
    }
    switch (W) {
#define X(w) case w: RFX_LAUNCH((k_sk_hist<w, DESC>), grid, dim3(SKT), 0, args...); break;
        RFX_SK_W_CASES(X)
#undef X
        default: RFX_LAUNCH((k_sk_hist<19, DESC>), grid, dim3(SKT), 0, args...); break;
    }
    return RFX_OK;
}

template <int W, bool DESC, bool WIDE, class... Args>
static int launch_sk_scatter_w(rfx_ctx *ctx, dim3 grid, size_t lds, Args... args) {
    RFX_HIP(hipFuncSetAttribute((const void *)k_sk_scatter<W, DESC, WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RFX_LAUNCH((k_sk_scatter<W, DESC, WIDE>), grid, dim3(SKT), lds, args...);
    return RFX_OK;
}
template <bool DESC, bool WIDE, class... Args>
static int launch_sk_scatter(rfx_ctx *ctx, int W, dim3 grid, size_t lds, Args... args) {
    if constexpr (WIDE) {                  // the central window is 30 or 31 bases: W = 18 or 19
        if (W == 18) return launch_sk_scatter_w<18, DESC, true>(ctx, grid, lds, args...);
        return launch_sk_scatter_w<19, DESC, true>(ctx, grid, lds, args...);
    } else {
        switch (W) {
#define X(w) case w: return launch_sk_scatter_w<w, DESC, false>(ctx, grid, lds, args...);
            RFX_SK_W_CASES(X)
#undef X
            default: return launch_sk_scatter_w<19, DESC, false>(ctx, grid, lds, args...);
        }
    }
}

// level 1 of the record path: reads -> records bucketed by `lv` (radix digit or owner).
// *out_recs (workspace slot `ws_slot`, or the caller's buffer d_dst of cap_dst records) receives
// the records, d_seg_off[nb+1] their bucket offsets; *n_recs the total.
template <bool WIDE>
int records_from_reads(rfx_ctx *ctx, const ReadSrc &rsrc, const Level &lv, bool use_ws, int ws_slot,
                       std::conditional_t<WIDE, WRec, Rec> *d_dst, int64_t cap_dst, uint64_t *d_seg_off,
                       std::conditional_t<WIDE, WRec, Rec> **out_recs, int64_t *n_recs,
                       const char *hn, const char *pn) {
    using Rec = std::conditional_t<WIDE, WRec, ::Rec>;
    const int nb = lv.n_owners > 0 ? lv.n_owners : (1 << lv.bits);
    const int W = rsrc.k - SK_M + 1;
    const size_t sk_lds = (size_t)nb * (SKB * sizeof(Rec) + 16);
    // two workgroups fit a CU when the rings are small; four times as many are launched then (the rest queue
    // behind the first and even out the tail: hist1 5.0 -> 4.6 ms)
    const int per_cu = sk_lds <= 80 * 1024 ? 8 : 1;
    const unsigned G = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rsrc.n_threads, SKT), (int64_t)ctx->num_cu * per_cu));
    DevBuf bh, scanned;
    RFX_ALLOC(bh, uint64_t, (size_t)nb * G);
    RFX_ALLOC(scanned, uint64_t, (size_t)nb * G + 1);
    // run descriptors (hist -> scatter) live in the workspace slot the records do not use yet
    uint32_t *desc = nullptr;
    const bool want_desc = lv.n_owners <= 64 && count_tuning().sk_desc;
    // (records into the caller's buffer: both slots are free; owner mode adds two words of owners)
    if (want_desc) desc = (uint32_t *)ctx->ws_get(use_ws && ws_slot == 1 ? 0 : 1, (size_t)(3 + SKD) * 4 * (size_t)rsrc.n_threads);
    {
        ScopedTimer t(ctx, hn);
        if (desc) RFX_TRY((launch_sk_hist<true, WIDE>(ctx, W, dim3(G), rsrc, lv, bh.as<uint64_t>(), desc)));
        else RFX_TRY((launch_sk_hist<false, WIDE>(ctx, W, dim3(G), rsrc, lv, bh.as<uint64_t>(), (uint32_t *)nullptr)));
    }
    RFX_TRY(exclusive_scan_u64(ctx, bh.as<uint64_t>(), scanned.as<uint64_t>(), (int64_t)nb * G));
    RFX_TRY(bin_offsets(ctx, scanned.as<uint64_t>(), nb, (int64_t)G, d_seg_off));
    uint64_t R = 0;
    RFX_HIP(hipMemcpyAsync(&R, scanned.as<uint64_t>() + (size_t)nb * G, 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_TRY(sync_checked(ctx));
    *n_recs = (int64_t)R;
    Rec *dst = d_dst;
    if (use_ws) {
        dst = (Rec *)ctx->ws_get(ws_slot, (size_t)R * sizeof(Rec));
        if (!dst) { ctx->last_error = "workspace allocation failed"; return RFX_E_HIP; }
    } else if (!dst || (int64_t)R > cap_dst) {
        return RFX_E_CAP;                      // caller's buffer missing or too small: *n_recs holds the need
    }
    {
        ScopedTimer t(ctx, pn);
        if (desc) RFX_TRY((launch_sk_scatter<true, WIDE>(ctx, W, dim3(G), sk_lds, rsrc, lv, scanned.as<uint64_t>(), dst, (const uint32_t *)desc)));
        else RFX_TRY((launch_sk_scatter<false, WIDE>(ctx, W, dim3(G), sk_lds, rsrc, lv, scanned.as<uint64_t>(), dst, (const uint32_t *)nullptr)));
    }
    *out_recs = dst;
    return RFX_OK;
}

// level 1 of the record path in one sweep (k_sk_onesweep): -> records in workspace slot `ws_slot`, bucket b in
// [d_seg_begin[b], d_seg_end[b]).  *done = false: a region overflowed, nothing is valid, take the two-pass form.
template <bool WIDE>
int records_onesweep(rfx_ctx *ctx, const ReadSrc &rsrc_in, const Level &lv, int ws_slot, uint64_t *d_seg_begin,
                     uint64_t *d_seg_end, std::conditional_t<WIDE, WRec, Rec> **out_recs, int64_t *n_recs, bool *done,
                     const char *hn, const char *pn, std::conditional_t<WIDE, WRec, Rec> *d_dst, int64_t cap_dst) {
    using Rec = std::conditional_t<WIDE, WRec, ::Rec>;
    const CountTuning tune = count_tuning();
    *done = false;
    const int nb = 1 << lv.bits;
    const int W = rsrc_in.k - SK_M + 1;
    // 32 windows per thread (seg_runs; 16 in rounds 1-2) up to 512 buckets.  The k = 33..63 records keep 16.
    const bool seg32 = !WIDE && nb <= 512;
    ReadSrc rsrc = rsrc_in;
    if (seg32) {
        rsrc.segs = rsrc.nk > 0 ? (rsrc.nk + 31) / 32 : 1;
        rsrc.n_threads = rsrc.n_reads * rsrc.segs;
    }
    const int OST = seg32 ? OsGeo<32, false>::T : SKT;            // threads per workgroup of the sweep = segments per tile
    const int64_t ntile = ceil_div(rsrc.n_threads, OST);
    const int64_t ntile_s = ceil_div(rsrc.n_threads, SKT);        // (the sampled histogram keeps tiles of SKT segments)
    // two workgroups per CU (one for the 32-byte records); fewer on small inputs (every workgroup holds three extents
    // per bucket: at least 32 tiles each)
    const int per_cu = WIDE ? 1 : 2;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(OS_MAXG, (int64_t)ctx->num_cu * per_cu),
                                                                std::max<int64_t>(std::min<int64_t>(ntile, 64), ntile / 32)));
    int sample = 32;
    if (ntile_s < 64 * (int64_t)sample) sample = (int)std::max<int64_t>(1, ntile_s / 64);      // small inputs: at least 64 tiles
    const int64_t n_sampled = ceil_div(ntile_s, sample);
    const int cap_pct = tune.sk_onesweep_cap;
    DevBuf hist, reg_start, reg_cap, cursor, totals, holes;
    RFX_HIP(hist.alloc((size_t)nb * 8 + 16, ctx->stream));                 // + the overflow flag
    RFX_ALLOC(reg_start, uint64_t, nb + 1);
    RFX_ALLOC(reg_cap, uint32_t, nb);
    RFX_ALLOC(cursor, unsigned long long, (size_t)nb * OS_CSTRIDE);
    RFX_HIP(totals.alloc(24, ctx->stream));
    RFX_ALLOC(holes, uint64_t, (size_t)nb * OS_HOLES * G);
    RFX_HIP(hipMemsetAsync(hist.p, 0, (size_t)nb * 8 + 16, ctx->stream));
    int *d_overflow = (int *)(hist.as<unsigned long long>() + nb);
    {
        ScopedTimer t(ctx, hn);
        const dim3 gs((unsigned)std::min<int64_t>(n_sampled, (int64_t)ctx->num_cu * 8));
        if constexpr (WIDE) {
            if (W == 18) RFX_LAUNCH((k_sk_sample_hist<18, 16, true>), gs, dim3(SKT), 0, rsrc, lv, sample, hist.as<unsigned long long>());
            else RFX_LAUNCH((k_sk_sample_hist<19, 16, true>), gs, dim3(SKT), 0, rsrc, lv, sample, hist.as<unsigned long long>());
        } else switch (W) {
#define X(w) case w: if (seg32) RFX_LAUNCH((k_sk_sample_hist<w, 32>), gs, dim3(SKT), 0, rsrc, lv, sample, hist.as<unsigned long long>()); \
                     else RFX_LAUNCH((k_sk_sample_hist<w>), gs, dim3(SKT), 0, rsrc, lv, sample, hist.as<unsigned long long>()); break;
            RFX_SK_W_CASES(X)
            default: X(19)
#undef X
        }
        RFX_LAUNCH(k_plan_regions, dim3(1), dim3(1024), 0, hist.as<unsigned long long>(), nb,
                   (double)ntile_s / (double)n_sampled, G, cap_pct, (double)ntile, reg_start.as<uint64_t>(), reg_cap.as<uint32_t>(),
                   cursor.as<unsigned long long>(), totals.as<unsigned long long>());
    }
    unsigned long long h_tot[3] = {0, 0, 0};
    RFX_HIP(hipMemcpyAsync(h_tot, totals.p, 24, hipMemcpyDeviceToHost, ctx->stream));
    RFX_TRY(sync_checked(ctx));
    const uint32_t ose = (uint32_t)h_tot[2];
    if (ose == 0) {                       // one bucket takes more of a tile than the largest extent: two passes straight away
        if (tune.trace) fprintf(stderr, "one-sweep level 1: not tried (the sample puts too much on one bucket)\n");
        return RFX_OK;
    }
    int ose_shift = 0;
    while ((1u << ose_shift) < ose) ose_shift++;
    Rec *dst = d_dst;
    if (d_dst) {                          // the caller's buffer (the regions with their slack must fit): *n_recs = the need
        if ((int64_t)h_tot[0] > cap_dst) { *n_recs = (int64_t)h_tot[0]; return RFX_E_CAP; }
    } else {
        dst = (Rec *)ctx->ws_get(ws_slot, (size_t)h_tot[0] * sizeof(Rec));
        if (!dst) { ctx->last_error = "workspace allocation failed"; return RFX_E_HIP; }
    }
    const OneSweep os{reg_start.as<uint64_t>(), reg_cap.as<uint32_t>(), cursor.as<unsigned long long>(), holes.as<uint64_t>(), d_overflow,
                      (uint64_t)h_tot[0], hist.as<unsigned long long>() + nb + 1, ose, (uint32_t)ose_shift};
    const size_t lds = (size_t)nb * (SKB * sizeof(Rec) + 24);
    {
        ScopedTimer t(ctx, pn);
        if constexpr (WIDE) {                  // the central window is 30 or 31 bases: W = 18 or 19
            if (W == 18) {
                RFX_HIP(hipFuncSetAttribute((const void *)k_sk_onesweep<18, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                RFX_LAUNCH((k_sk_onesweep<18, true>), dim3((unsigned)G), dim3(SKT), lds, rsrc, lv, os, dst);
            } else {
                RFX_HIP(hipFuncSetAttribute((const void *)k_sk_onesweep<19, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                RFX_LAUNCH((k_sk_onesweep<19, true>), dim3((unsigned)G), dim3(SKT), lds, rsrc, lv, os, dst);
            }
        } else {
            switch (W) {
#define X(w) case w: if (seg32) { \
                         RFX_HIP(hipFuncSetAttribute((const void *)k_sk_onesweep<w, false, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                         RFX_LAUNCH((k_sk_onesweep<w, false, 32>), dim3((unsigned)G), dim3(OST), lds, rsrc, lv, os, dst); \
                     } else { \
                         RFX_HIP(hipFuncSetAttribute((const void *)k_sk_onesweep<w>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                         RFX_LAUNCH((k_sk_onesweep<w>), dim3((unsigned)G), dim3(SKT), lds, rsrc, lv, os, dst); \
                     } break;
                RFX_SK_W_CASES(X)
                default: X(19)
#undef X
            }
        }
        RFX_LAUNCH(k_fix_holes<Rec>, dim3((unsigned)nb), dim3(FH_T), 0, os, G, dst, d_seg_begin, d_seg_end,
                   totals.as<unsigned long long>());
    }
    int h_flag[2] = {0, 0};
    RFX_HIP(hipMemcpyAsync(h_tot, totals.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    RFX_HIP(hipMemcpyAsync(h_flag, d_overflow, 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_TRY(sync_checked(ctx));
    const int h_over = h_flag[0];
    if (h_flag[1]) ctx->timing["stat_l1_void_rounds"].launches += 1;     // a round outran its two extents (not: a region ran out)
    if (tune.trace)
        fprintf(stderr, "one-sweep level 1: %llu records in regions of %llu (sample 1/%d, %d workgroups, extents of %u)%s\n", h_tot[1], h_tot[0], sample, G, ose,
                h_over ? " -- a region overflowed: two passes instead" : "");
    if (h_over == 2) { ctx->last_error = "one-sweep level 1: holes and tail records do not balance"; return RFX_E_STATE; }
    if (h_over) return RFX_OK;
    *out_recs = dst;
    *n_recs = (int64_t)h_tot[1];
    ctx->timing["stat_records"].launches += (int64_t)h_tot[1];           // records the sweep wrote (the merged cut's yardstick)
    *done = true;
    return RFX_OK;
}

// reads -> records -> count (the default for k = 28..31)
int count_reads_superkmer(rfx_ctx *ctx, const ReadStore *reads, int min_cov, int max_cov, int twin,
                          uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap, int64_t *out_n,
                          int64_t *out_distinct, bool pair_out) {
    ctx->timing.clear();
    ReadSrc rsrc = make_read_src(reads);
    const int64_t n = instances_of(reads, rsrc);
    if (out_n) *out_n = 0;
    if (out_distinct) *out_distinct = 0;
    if (n <= 0) return RFX_OK;
    std::vector<int> bits;
    plan_levels(n, true, bits, 16384.0);           // measured best for the record leaf with double hashing + pre-split
    // (20 bits and more put 1024 bins on level 1 and one workgroup per CU there, the rings fill the LDS.  Measured on one
    // GPU: 20 Gbp of the 4.64 Mbp genome 138.8 ms with 10 + 10 bits, 131.7 with 9 + 10 and leaves twice as large, 139
    // with three levels; 18.75 Gbp of a 400 Mbp genome -- 2.5e9 distinct k-mers, a human-scale share -- 238 ms with
    // 10 + 10, 254 with 9 + 10: the leaves of a deep data set want to be small, so the plan stays as it is)
    Level lv{};
    lv.bits = bits[0];
    StageArena stage_arena(ctx, ((size_t)64 << 20) + (size_t)n / 8);
    DevBuf segA, segB;
    RFX_ALLOC(segA, uint64_t, (size_t)(1 << lv.bits) + 1);
    Rec *recs = nullptr;
    int64_t R = 0;
    // level 1 in one sweep when the input is large enough for a sampled histogram to size the regions (and another
    // level follows: the leaves want gap-free buckets); RFX_SK_ONESWEEP=0 two passes always, =2 one sweep at any size
    bool swept = false;
    DevBuf segE;
    if (bits.size() >= 2 && sweep_level1(count_tuning(), rsrc.n_threads)) {
        RFX_ALLOC(segE, uint64_t, 1 << lv.bits);
        RFX_TRY(records_onesweep(ctx, rsrc, lv, 0, segA.as<uint64_t>(), segE.as<uint64_t>(), &recs, &R, &swept, "hist1", "part1"));
    }
    if (!swept) RFX_TRY(records_from_reads(ctx, rsrc, lv, true, 0, nullptr, 0, segA.as<uint64_t>(), &recs, &R, "hist1", "part1"));
    return count_records_levels(ctx, recs, R, 0, bits, 1, lv.bits, &segA, &segB, (int64_t)1 << lv.bits, reads->k,
                                min_cov, max_cov, twin, d_out_keys, d_out_counts, cap, out_n, out_distinct, pair_out,
                                swept ? segE.as<uint64_t>() : nullptr);
}

// multi-GPU, record form: bucket this rank's reads by the OWNER of each run's minimiser
// (owner = mulhi(hash(minimiser), n_owners)) -- the exchange then ships ~2.6 B per instance
int bucket_records_by_owner(rfx_ctx *ctx, const ReadStore *reads, int n_owners, void *d_out, int64_t cap_records,
                            int64_t *d_owner_off, int64_t *h_owner_off, int64_t *out_n_records) {
    StageArena stage_arena(ctx, (size_t)256 << 20);       // temporaries of this call (see StageArena)
    if (n_owners < 1 || n_owners > 64 || !superkmer_enabled(reads->k)) return RFX_E_ARG;
    ReadSrc rsrc = make_read_src(reads);
    if (out_n_records) *out_n_records = 0;
    if (rsrc.nk <= 0 || reads->n_reads <= 0) return zero_owner_offsets(ctx, n_owners, d_owner_off, h_owner_off);
    Level lv{};
    lv.n_owners = n_owners;
    Rec *recs = nullptr;
    int64_t R = 0;
    int st = records_from_reads(ctx, rsrc, lv, false, 0, (Rec *)d_out, cap_records,
                                reinterpret_cast<uint64_t *>(d_owner_off), &recs, &R, "hist1", "part1");
    if (out_n_records) *out_n_records = R;
    if (st != RFX_OK) return st;
    if (h_owner_off) {
        RFX_HIP(hipMemcpyAsync(h_owner_off, d_owner_off, (size_t)(n_owners + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        RFX_TRY(sync_checked(ctx));
    }
    return RFX_OK;
}

// One owner's bucket lies in S consecutive bins of the sweep, bin i gap-free in [seg_begin, seg_end) with the regions' slack
// between the bins: the records that lie beyond the bucket's own length are moved into the gaps before it, so that the
// bucket is ONE run [begin, begin + total) -- one message per peer, as with the two-pass form.  Sources lie at or
// beyond the cut, destinations before it.  grid (owners, chunks).
template <class RT>
static __global__ __launch_bounds__(1024) void k_close_gaps(RT *__restrict__ recs, const uint64_t *__restrict__ seg_begin,
                                                     const uint64_t *__restrict__ seg_end, int S, uint64_t *__restrict__ out_begin,
                                                     uint64_t *__restrict__ out_end, int *__restrict__ fault) {
    __shared__ uint64_t slo[512], dlo[512], spre[513], dpre[513];       // (S <= 512: one owner and all the sweep's bins)
    const int o = blockIdx.x;
    const uint64_t *sb = seg_begin + (size_t)o * S, *se = seg_end + (size_t)o * S;
    if (threadIdx.x == 0) {
        uint64_t R = 0;
        for (int i = 0; i < S; i++) R += se[i] - sb[i];
        const uint64_t cut = sb[0] + R;
        spre[0] = dpre[0] = 0;
        for (int i = 0; i < S; i++) {
            const uint64_t lo = sb[i] > cut ? sb[i] : cut;
            slo[i] = lo;
            spre[i + 1] = spre[i] + (se[i] > lo ? se[i] - lo : 0);
            uint64_t g0 = se[i], g1 = i + 1 < S ? sb[i + 1] : se[i];
            if (g1 > cut) g1 = cut;
            dlo[i] = g0;
            dpre[i + 1] = dpre[i] + (g1 > g0 ? g1 - g0 : 0);
        }
        if (spre[S] != dpre[S]) *fault = 1;                      // (never: both count the bucket's records beyond the cut)
        if (blockIdx.y == 0) { out_begin[o] = sb[0]; out_end[o] = cut; }
    }
    __syncthreads();
    const uint64_t M = spre[S] < dpre[S] ? spre[S] : dpre[S];
    for (uint64_t k = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; k < M; k += (uint64_t)gridDim.y * blockDim.x) {
        int i = 0, j = 0;                                               // the last range that starts at or before k
        for (int st = S >> 1; st > 0; st >>= 1) {
            if (spre[i + st] <= k) i += st;
            if (dpre[j + st] <= k) j += st;
        }
        recs[dlo[j] + (k - dpre[j])] = recs[slo[i] + (k - spre[i])];
    }
}

// The same by level 1's ONE SWEEP (round 3).  The sweep wants a bin to receive a handful of records per round (8-slot
// rings, extents of 64), and an owner bucket of a rank of 8 receives hundreds -- so every owner's bucket is cut into
// 2^sub_bits bins by the top bits of the record header (512 bins in all; the receiver does not care which bin a record
// came through), and k_close_gaps then makes every owner's bins one run: owner b = records [h_begin[b], h_end[b]) of
// d_out, with slack between the owners.  *done = false: not tried or void (small input, skew, a region that
// overflowed): the caller takes bucket_records_by_owner.  RFX_E_CAP: *out_n_records = the records d_out must hold
// (regions + slack).
template <bool WIDE>
static int owner_sweep(rfx_ctx *ctx, const ReadSrc &rsrc, int n_owners, void *d_out, int64_t cap_records, int64_t *h_begin,
                       int64_t *h_end, int64_t *out_n_records, bool *done) {
    using RT = std::conditional_t<WIDE, WRec, Rec>;
    *done = false;
    if (rsrc.nk <= 0 || rsrc.n_reads <= 0 || !sweep_level1(count_tuning(), rsrc.n_threads)) return RFX_OK;
    StageArena stage_arena(ctx, (size_t)256 << 20);       // temporaries of this call (see StageArena)
    int obits = 0;
    while ((1 << obits) < n_owners) obits++;
    Level lv{};
    lv.n_owners = n_owners;
    lv.sub_bits = 9 - obits;                              // >= 3
    lv.bits = 9;
    const int nb = 1 << lv.bits, S = 1 << lv.sub_bits;
    DevBuf segB, segE, ob, oe, flt;
    RFX_ALLOC(segB, uint64_t, nb + 1);
    RFX_ALLOC(segE, uint64_t, nb);
    RFX_ALLOC(ob, uint64_t, n_owners);
    RFX_ALLOC(oe, uint64_t, n_owners);
    RFX_HIP(flt.alloc(4, ctx->stream));
    RFX_HIP(hipMemsetAsync(flt.p, 0, 4, ctx->stream));
    RT *recs = nullptr;
    int64_t R = 0;
    bool swept = false;
    int st = records_onesweep<WIDE>(ctx, rsrc, lv, 0, segB.as<uint64_t>(), segE.as<uint64_t>(), &recs, &R, &swept, "hist1", "part1",
                                    (RT *)d_out, cap_records);
    if (out_n_records) *out_n_records = R;
    if (st != RFX_OK || !swept) return st;
    {
        ScopedTimer t(ctx, "part1");
        RFX_LAUNCH(k_close_gaps<RT>, dim3((unsigned)n_owners, 16), dim3(1024), 0, recs, segB.as<uint64_t>(),
                   segE.as<uint64_t>(), S, ob.as<uint64_t>(), oe.as<uint64_t>(), flt.as<int>());
    }
    int h_fault = 0;
    static_assert(sizeof(int64_t) == sizeof(uint64_t), "offsets");
    RFX_HIP(hipMemcpyAsync(h_begin, ob.p, (size_t)n_owners * 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_HIP(hipMemcpyAsync(h_end, oe.p, (size_t)n_owners * 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_HIP(hipMemcpyAsync(&h_fault, flt.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    RFX_TRY(sync_checked(ctx));
    if (h_fault) { ctx->last_error = "owner sweep: gaps and tail records do not balance"; return RFX_E_STATE; }
    *done = true;
    return RFX_OK;
}

int bucket_records_by_owner_sweep(rfx_ctx *ctx, const ReadStore *reads, int n_owners, void *d_out, int64_t cap_records,
                                  int64_t *h_begin, int64_t *h_end, int64_t *out_n_records, bool *done) {
    *done = false;
    if (n_owners < 1 || n_owners > 64 || !superkmer_enabled(reads->k)) return RFX_E_ARG;
    return owner_sweep<false>(ctx, make_read_src(reads), n_owners, d_out, cap_records, h_begin, h_end, out_n_records, done);
}

// ragged reads (d_read_len != nullptr): nk = the k-mers of the longest read (the segments per read), every read
// emits nk_of_wide(its length) of them (read_nk<true>)
ReadSrc wide_read_src(const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                      const uint32_t *d_read_len, int ec) {
    ReadSrc s{};
    const int c = (k & 1) ? 31 : 30;               // central window; (k - c) / 2 bases of the k-mer on either side
    s.words = d_words; s.n_reads = n_reads; s.wpr = wpr;
    s.wfl = (k - c) / 2;
    s.fc = fc + s.wfl; s.k = c;
    s.nk = (int)nk;
    s.segs = s.nk > 0 ? (s.nk + PK - 1) / PK : 1;
    s.n_threads = s.n_reads * s.segs;
    s.len_arr = d_read_len; s.ec = ec;
    return s;
}

// multi-GPU, k = 33..63: the 32-byte records grouped by the owner of their minimiser (~5 B per instance
// across the exchange instead of 16), and the count of records that arrived
int bucket_wide_records_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                                 int n_owners, void *d_out, int64_t cap_records, int64_t *d_owner_off, int64_t *h_owner_off,
                                 int64_t *out_n_records, const uint32_t *d_read_len, int ec) {
    StageArena stage_arena(ctx, (size_t)256 << 20);       // temporaries of this call (see StageArena)
    if (n_owners < 1 || n_owners > 64 || k < 33 || k > 63) return RFX_E_ARG;
    if (out_n_records) *out_n_records = 0;
    if (nk <= 0 || n_reads <= 0) return zero_owner_offsets(ctx, n_owners, d_owner_off, h_owner_off);
    ReadSrc rsrc = wide_read_src(d_words, n_reads, wpr, nk, k, fc, d_read_len, ec);
    Level lv{};
    lv.n_owners = n_owners;
    WRec *recs = nullptr;
    int64_t R = 0;
    const int st = records_from_reads<true>(ctx, rsrc, lv, false, 0, (WRec *)d_out, cap_records,
                                            reinterpret_cast<uint64_t *>(d_owner_off), &recs, &R, "hist1", "part1");
    if (out_n_records) *out_n_records = R;
    if (st != RFX_OK) return st;
    if (h_owner_off) {
        RFX_HIP(hipMemcpyAsync(h_owner_off, d_owner_off, (size_t)(n_owners + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        RFX_TRY(sync_checked(ctx));
    }
    return RFX_OK;
}

// the same for the 32-byte records of k = 33..63 (bucket_wide_records_by_owner)
int bucket_wide_records_by_owner_sweep(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                                       int n_owners, void *d_out, int64_t cap_records, int64_t *h_begin, int64_t *h_end,
                                       int64_t *out_n_records, bool *done, const uint32_t *d_read_len, int ec) {
    *done = false;
    if (n_owners < 1 || n_owners > 64 || k < 33 || k > 63) return RFX_E_ARG;
    if (nk <= 0 || n_reads <= 0) return RFX_OK;
    return owner_sweep<true>(ctx, wide_read_src(d_words, n_reads, wpr, nk, k, fc, d_read_len, ec), n_owners, d_out, cap_records, h_begin, h_end,
                             out_n_records, done);
}

// the instantiations rfx_kmer.hip calls (rfx_count.h)
template decltype(records_from_reads<false>) records_from_reads<false>;
template decltype(records_from_reads<true>) records_from_reads<true>;
template decltype(records_onesweep<false>) records_onesweep<false>;
template decltype(records_onesweep<true>) records_onesweep<true>;

}  // namespace rfx
