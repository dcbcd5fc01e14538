// rfx_dedup.hip -- contig RC de-duplication: P/ReflexivDSDynamicKmerDedup.java on the GPU.
//
// The reference's driver (`assemblyFromKmer`, :138-339) runs three rounds of: marker 31-mers of every contig of >= 300 bases
// (seeds at the block starts, probes at a few windows; round 1 probes the reverse complement only, rounds 2 and 3 both
// strands: :2674-3096, :2206-2673) -> sort -> DSMarkerKmerSelection (:1788-1870: a probe of a shorter contig that meets a
// seed of the same 31-mer names the pair) -> groupBy().count() >= 2 -> the shorter contig is sent to its target
// (:3186-3207, :3097-3132) -> the removal class merges the contigs that share a target into the longest by 15-mer seed
// voting (`merge2RCContigs`, :1462-1557 / :565-728), an unmatched short contig goes back to the pool.
//
// Here: contigs live in HBM PACKED, 2 bits per base, 32 bases per 64-bit word, every contig on a word, every bit past its last
// base 0 (rfx_contigs_packed); the unit of work of every kernel that touches bases is a word, read
// through the helpers of rfx_dedup_words.h (one or two word loads and two shifts for any 32-base window of either strand).
// Kernels: k_dd_markers (one thread per seed / probe: one window), the library's stable radix sort on the sign-flipped 31-mer,
// k_dd_select (the owner of an equal-31-mer run walks it: the reference's one-row `LongestKmer` and its `shorterKmer` list
// never outlive a run of equal k-mers except to be compared with the next run's first seed), a second sort + k_dd_pair_runs
// for count >= 2; per step of a round k_dd_seed_insert_b (open-addressing tables, the HashMap's "a later position replaces an
// earlier one" as atomicMax), k_dd_query_b (all 15-mers of the short contigs, either strand), one sort of the distances,
// k_dd_vote (the reference's sequential vote, a wave per merge: it is a scan with a data-dependent anchor) and k_dd_emit: one
// thread per OUTPUT word of a merged contig (one descriptor of two pieces: long + flank or flank + long) or of a contig of
// the round's output (a descriptor of one piece).  The pairing of contigs with their targets is bookkeeping on contig IDS (a
// few numbers per contig) and runs on the host between the kernels, as the Spark driver's plan does in the reference.
// Order contract as everywhere: one logical partition, stable sorts on the signed column, union =
// left then right, groupBy().count() ascending, zipWithIndex = position.
//
// The entry points: rfx_dev_contigs_pack / _unpack / _from_text / _to_text and rfx_dev_dedup_contigs on the caller's device
// arrays; rfx_dedup_contigs and rfx_dedup_contig_text are pack (or from-text) -> the same kernels -> unpack / to-text.
#include <algorithm>
#include <string>
#include <vector>
#include "rfx_internal.h"
#include "rfx_dedup_words.h"

using namespace rfx;

namespace {

constexpr int M31 = 31;

__host__ __device__ __forceinline__ int64_t dd_attr3(int marker, int64_t left, int64_t right) {     // :2908-2934
    if (left >= 500000000) left = 500000000; else if (left <= -500000000) left = 1000000000; else if (left < 0) left = 500000000 - left;
    if (right >= 1000000000) right = 1000000000; else if (right <= -1000000000) right = 2000000000; else if (right < 0) right = 1000000000 - right;
    return (int64_t)(((uint64_t)marker << 62) | ((uint64_t)(uint32_t)left << 32) | (uint64_t)(uint32_t)right);
}
__device__ __forceinline__ int dd_marker(int64_t a) { return (int)((uint64_t)a >> 62); }
__device__ __forceinline__ int32_t dd_left(int64_t a) {               // getLeftMarker :1882-1892
    int32_t l = (int32_t)((uint64_t)a >> 32) & ~(3 << 30);
    if (l > 500000000) l = 500000000 - l;
    return l;
}
__device__ __forceinline__ int32_t dd_right(int64_t a) {              // getRightMarker :1894-1902
    int32_t r = (int32_t)a;
    if (r > 1000000000) r = 1000000000 - r;
    return r;
}

// probe windows of a contig of L bases (getRCKmerProbBinary :2713-2875): up to five [a, b)
__host__ __device__ inline int dd_windows(int64_t L, int64_t w[5][2]) {
    int n = 0;
    const int64_t M = M31;
    if (L >= 4000) {
        w[n][0] = 0; w[n++][1] = M; w[n][0] = 1000 - M + 1; w[n++][1] = 1000; w[n][0] = (L - 2 * M) / 2; w[n][1] = w[n][0] + M; n++;
        w[n][0] = L - 1000 - M + 1; w[n++][1] = L - 1000; w[n][0] = L - 2 * M; w[n++][1] = L - M;
    } else if (L >= 2000) {
        w[n][0] = 0; w[n++][1] = M; w[n][0] = 600 - M + 1; w[n++][1] = 600; w[n][0] = (L - 2 * M) / 2; w[n][1] = w[n][0] + M; n++;
        w[n][0] = L - 600 - M + 1; w[n++][1] = L - 600; w[n][0] = L - 2 * M; w[n++][1] = L - M;
    } else {
        w[n][0] = 0; w[n++][1] = M; w[n][0] = (L - 2 * M) / 3; w[n][1] = w[n][0] + M; n++;
        w[n][0] = (L - 2 * M) * 2 / 3; w[n][1] = w[n][0] + M; n++; w[n][0] = L - 2 * M; w[n++][1] = L - M;
    }
    return n;
}
// where the p-th probe position of a contig of L bases lies: the windows of dd_windows walked without the array (registers only)
__host__ __device__ inline int64_t dd_probe_at(int64_t L, int64_t p) {
    const int64_t M = M31;
    if (L >= 2000) {
        const int64_t side = L >= 4000 ? 1000 : 600;
        if (p < M) return p;
        p -= M;
        if (p < M - 1) return side - M + 1 + p;
        p -= M - 1;
        if (p < M) return (L - 2 * M) / 2 + p;
        p -= M;
        if (p < M - 1) return L - side - M + 1 + p;
        p -= M - 1;
        return L - 2 * M + p;
    }
    if (p < M) return p;
    p -= M;
    if (p < M) return (L - 2 * M) / 3 + p;
    p -= M;
    if (p < M) return (L - 2 * M) * 2 / 3 + p;
    p -= M;
    return L - 2 * M + p;
}
inline int64_t dd_seed_count(int64_t L) { return L < 300 ? 0 : (L - 1) / 31 + (L % 31 == 0 ? 1 : 0); }
inline int64_t dd_probe_positions(int64_t L) {
    if (L < 300) return 0;
    int64_t w[5][2];
    const int n = dd_windows(L, w);
    int64_t t = 0;
    for (int i = 0; i < n; i++) t += w[i][1] - w[i][0];
    return t;
}

// one thread per marker row, in the reference's emission order: contig after contig; inside a contig the seeds (block
// starts, ascending), then window after window, position after position (forward probe, then its reverse complement, when
// both strands are probed).  A marker is one 32-base window of the packed contig.
__global__ __launch_bounds__(256) void k_dd_markers(const uint64_t *__restrict__ pool, const int64_t *__restrict__ cwoff,
                                                    const int64_t *__restrict__ clen, const int64_t *__restrict__ cid,
                                                    const int64_t *__restrict__ moff, int64_t n_contigs, int64_t n_markers, int both,
                                                    uint64_t *__restrict__ key, uint32_t *__restrict__ val, int64_t *__restrict__ attr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_markers) return;
    const int64_t c = pk_find(moff, n_contigs, t), L = clen[c];
    const uint64_t *s = pool + cwoff[c];
    int64_t j = t - moff[c];
    const int64_t nb = (L - 1) / 31 + 1, nseed = (nb - 1) + (L % 31 == 0 ? 1 : 0);
    uint64_t k;
    int64_t a;
    if (j < nseed) {
        k = dd_mer31(s, L, 31 * j);
        a = dd_attr3(1, L, (int32_t)cid[c]);
    } else {
        j -= nseed;
        const int per = both ? 2 : 1;
        const int64_t pos = dd_probe_at(L, j / per);
        const uint64_t f = dd_mer31(s, L, pos);
        k = (both && (j % per) == 0) ? f : dd_mer31_rc(f);
        a = dd_attr3(2, L, (int32_t)cid[c]);
    }
    key[t] = k ^ 0x8000000000000000ull;                   // sort("kmerBinary") orders the SIGNED long
    val[t] = (uint32_t)t;
    attr[t] = a;
}

// DSMarkerKmerSelection.call (:1796-1868) on the sorted rows: the thread that owns the head of an equal-31-mer run walks it.
// A probe ahead of the run's first seed meets that seed (`s` of the reference, the row that opens the new k-mer); a probe
// behind it meets the run's longest seed (`LongestKmer` when the list is flushed).  pair[q] = the pair id or -1.
__global__ __launch_bounds__(256) void k_dd_select(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                   const int64_t *__restrict__ attr, int64_t n, int64_t *__restrict__ pair) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    if (q > 0 && key[q - 1] == key[q]) return;
    int64_t e = q;
    int64_t first = -1, best_a = 0, first_a = 0;
    while (e < n && key[e] == key[q]) {
        const int64_t a = attr[val[e]];
        if (dd_marker(a) == 1) {
            if (first < 0) { first = e; first_a = a; best_a = a; }
            else if (dd_left(a) > dd_left(best_a)) best_a = a;
        }
        e++;
    }
    for (int64_t i = q; i < e; i++) {
        const int64_t a = attr[val[i]];
        int64_t out = -1;
        if (dd_marker(a) != 1 && first >= 0) {
            const int64_t ref = i < first ? first_a : best_a;
            const bool hit = dd_left(a) < dd_left(ref) || (dd_left(a) == dd_left(ref) && dd_right(a) > dd_right(ref));
            if (hit) out = (int64_t)(((uint64_t)(uint32_t)dd_right(a) << 32) | (uint64_t)(uint32_t)dd_right(ref));   // :1870-1880
        }
        pair[i] = out;
    }
}

// pair ids >= 0 -> compacted keys for the second sort (the rest are dropped)
__global__ __launch_bounds__(256) void k_dd_compact_pairs(const int64_t *__restrict__ pair, int64_t n, uint64_t *__restrict__ out,
                                                          unsigned long long *__restrict__ cnt) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n || pair[q] < 0) return;
    out[atomicAdd(cnt, 1ull)] = (uint64_t)pair[q];
}
// sorted pair ids -> the ids seen at least twice (groupBy().count() >= 2, :186-194)
__global__ __launch_bounds__(256) void k_dd_pair_runs(const uint64_t *__restrict__ key, int64_t n, uint64_t *__restrict__ out,
                                                      unsigned long long *__restrict__ cnt) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    if (q > 0 && key[q - 1] == key[q]) return;
    if (q + 1 < n && key[q + 1] == key[q]) out[atomicAdd(cnt, 1ull)] = key[q];
}

// ---- merge2RCContigs --------------------------------------------------------------------------------------------------
constexpr uint32_t DD_EMPTY = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t dd_hash(uint32_t k) { return (uint32_t)(((uint64_t)k * 0x9E3779B97F4A7C15ull) >> 24); }

// ---- the merges of a round, BATCHED (round 4).  Until round 3 every (short, long) pair was its own launch sequence with two
// host waits (93 us a pair: 4.7 s for the 50,000 pairs of a 100,000-contig set); now step j of a round takes the j-th short
// contig of EVERY group at once: one table region cut into per-merge tables, one seed-insert launch, one query launch whose
// hits carry their merge's number above the distance, ONE sort of all distances, one vote launch (a wave per merge), one
// readback of all votes, one emit launch for all the merged contigs.  Same arithmetic per merge, same order of the outputs.
struct MergeB {                        // one merge of a batch (device copy)
    const uint64_t *lng, *sh;          // packed words
    int64_t ln, sn;                    // bases
    int64_t toff;                      // its table inside the region (slots)
    uint32_t tmask;
    int32_t rc, min_votes, active;
    int64_t spre, qpre;                // first seed thread / first query thread of this merge
};
__device__ __forceinline__ int64_t dd_find(const MergeB *__restrict__ mb, int64_t nm, int64_t t, bool query) {
    int64_t lo = 0, hi = nm;           // the last merge whose first thread is <= t
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((query ? mb[mid].qpre : mb[mid].spre) <= t) lo = mid; else hi = mid;
    }
    return lo;
}
// the 15-mer seeds of the long contigs at 0, 15, 30 .. ln (the one at ln, when it is issued, lies wholly past the end: C, then A's)
__global__ __launch_bounds__(256) void k_dd_seed_insert_b(const MergeB *__restrict__ mb, int64_t nm, int64_t total, uint32_t *__restrict__ tkey,
                                                          int32_t *__restrict__ tpos) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const MergeB m = mb[dd_find(mb, nm, t, false)];
    const int64_t i = (t - m.spre) * 15;
    if (i > m.ln) return;
    const uint32_t k = dd_seed15(m.lng, m.ln, i, 0);
    uint32_t h = dd_hash(k) & m.tmask;
    for (;;) {
        const uint32_t old = atomicCAS(&tkey[m.toff + h], DD_EMPTY, k);
        if (old == DD_EMPTY || old == k) { atomicMax(&tpos[m.toff + h], (int32_t)(i + 1)); return; }     // HashMap.put: the later position stays
        h = (h + 1) & m.tmask;
    }
}
__global__ __launch_bounds__(256) void k_dd_query_b(const MergeB *__restrict__ mb, int64_t nm, int64_t total, const uint32_t *__restrict__ tkey,
                                                    const int32_t *__restrict__ tpos, uint64_t *__restrict__ dist,
                                                    unsigned long long *__restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t g = dd_find(mb, nm, t, true);
    const MergeB m = mb[g];
    if (!m.active) return;
    const int64_t i = t - m.qpre;
    if (i >= m.sn) return;
    const uint32_t k = dd_seed15(m.sh, m.sn, i, m.rc);
    uint32_t h = dd_hash(k) & m.tmask;
    for (;;) {
        const uint32_t kk = tkey[m.toff + h];
        if (kk == DD_EMPTY) return;
        if (kk == k) {
            const int32_t d = (int32_t)(i + 1) - tpos[m.toff + h];
            // the merge's number above the biased distance: one sort orders every merge's list
            dist[atomicAdd(cnt, 1ull)] = ((uint64_t)g << 33) | (uint64_t)((int64_t)d + 0x80000000ll);
            return;
        }
        h = (h + 1) & m.tmask;
    }
}
// seg[g] = first entry of merge g in the sorted list (seg[nm] = total)
__global__ __launch_bounds__(256) void k_dd_seg_bounds(const uint64_t *__restrict__ dist, int64_t total, int64_t nm, int64_t *__restrict__ seg) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > nm) return;
    const uint64_t want = (uint64_t)g << 33;
    int64_t lo = 0, hi = total;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (dist[mid] < want) lo = mid + 1; else hi = mid; }
    seg[g] = lo;
}
// The emission, by OUTPUT word: a descriptor is one output contig -- a merge (two pieces, each of either strand of a packed
// contig) or a copy (one piece) --, one thread per 64-bit word of it reads its 32 bases from dd_cat32 of the pieces (0 past the
// end: the last word comes out masked) and stores 8 bytes, contiguous across lanes.  pre = the descriptor's first thread.
struct EmitB { uint64_t *dst; DdSeg a, b; int64_t pre; };
__global__ __launch_bounds__(256) void k_dd_emit(const EmitB *__restrict__ eb, int64_t ne, int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    int64_t lo = 0, hi = ne;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (eb[mid].pre <= t) lo = mid; else hi = mid; }
    const EmitB e = eb[lo];
    const int64_t j = t - e.pre;
    if (j >= ((e.a.n + e.b.n + 31) >> 5)) return;
    e.dst[j] = dd_cat32(e.a, e.b, 32 * j);
}

// the vote over the sorted distances (:1478-1497 with 3 votes, :578-597 / :617-636 with 4): sequential by definition (the
// anchor of a run is the first distance that left the previous run)
__global__ __launch_bounds__(64) void k_dd_vote(const uint64_t *__restrict__ dist_all, const int64_t *__restrict__ seg, const MergeB *__restrict__ mb,
                                                int64_t total_1, int min_votes_1, int32_t *__restrict__ out_all) {
    // batched: block b votes on merge b's slice of the one sorted list (seg; the merge's number sits above bit 33 of every
    // entry); seg == nullptr: the single list of rounds 1-3's form
    const uint64_t *dist = dist_all;
    int64_t total = total_1;
    int min_votes = min_votes_1;
    int32_t *out = out_all;
    if (seg) {
        if (!mb[blockIdx.x].active) return;
        dist = dist_all + seg[blockIdx.x]; total = seg[blockIdx.x + 1] - seg[blockIdx.x]; min_votes = mb[blockIdx.x].min_votes; out = out_all + blockIdx.x;
    }
    // one wave: 64 distances per coalesced load, then the scan itself on wave-uniform values (readlane) -- the anchor chain
    // is sequential, the memory latency need not be (a thread walking the list alone paid ~13 ns a distance).  And a run
    // need not be walked at all: the list is sorted, so once an element and the LAST element of its block both lie within
    // one of the anchor, everything between them does, the run's end beyond the block is found by a 64-ary search (the
    // true overlap of two 2.6 Mbp contigs is one run of a million equal distances: 1.9 ms walked, four probes searched), and
    // the vote is won at a known element of it -- the first frequency f with f / total >= 0.3 and f >= min_votes.
    const int lane = threadIdx.x;
    auto val = [&](int64_t i) -> int32_t { return (int32_t)((int64_t)(dist[i] & 0x1FFFFFFFFull) - 0x80000000ll); };
    int64_t T = (int64_t)(0.3 * (double)total);
    if (T < 1) T = 1;
    while (T > 1 && (double)(T - 1) / (double)total >= 0.3) T--;
    while ((double)T / (double)total < 0.3) T++;
    if (T < (int64_t)min_votes) T = min_votes;
    int32_t lastDistance = 0, fin = -1;
    int64_t lastFrequency = 0;
    bool done = false;
    int64_t base = 0;
    while (base < total && !done) {
        const int64_t i = base + lane;
        const int32_t v = i < total ? val(i) : 0;
        const int cnt = (int)(total - base < 64 ? total - base : 64);
        const int32_t dl = __builtin_amdgcn_readlane(v, cnt - 1);
        int64_t next = base + cnt;
        for (int j = 0; j < cnt; j++) {
            const int32_t d = __builtin_amdgcn_readlane(v, j);
            if (d - lastDistance >= -1 && d - lastDistance <= 1) {
                if (dl - lastDistance <= 1) {
                    // the run covers the rest of this block; its end e beyond it
                    int64_t lo = base + cnt, hi = cnt == 64 ? total : lo;
                    while (lo < hi) {
                        const int64_t step = (hi - lo + 63) / 64;
                        const int64_t p = lo + (int64_t)lane * step;
                        const bool in_run = p < hi && val(p) - lastDistance <= 1;
                        const int m = (int)__popcll(__ballot(in_run));              // a prefix of the lanes (sorted)
                        if (m == 0) { hi = lo; break; }
                        const int64_t last_in = lo + (int64_t)(m - 1) * step;
                        const int64_t first_out = lo + (int64_t)m * step;
                        lo = last_in + 1;
                        if (m < 64 && first_out < hi) hi = first_out;
                    }
                    const int64_t start = base + j, added = lo - start;
                    if (lastFrequency + added >= T) { fin = val(start + (T - lastFrequency) - 1); done = true; }
                    lastFrequency += added;
                    next = lo;
                    break;
                }
                lastFrequency++;
                if (lastFrequency >= T) { fin = d; done = true; break; }
            } else { lastFrequency = 1; lastDistance = d; }
        }
        base = next;
    }
    if (lane == 0) *out = fin;
}

__global__ __launch_bounds__(256) void k_dd_fill(uint32_t *p, uint32_t v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- the packed set (rfx_contigs_packed) -------------------------------------------------------------------------------------
// The arrays in HBM -- the library's own, or a view of the caller's -- and, on the host, the offsets and lengths the plan works on.
struct DdSet {
    int64_t n = 0, words = 0;
    DevBuf w, woff, len;                       // words; n + 1 word offsets; n lengths in bases
    std::vector<int64_t> h_woff, h_len;
};
// A0 C1 G2, anything else 3 (nucleotideValue :453-465)
__device__ __forceinline__ uint64_t dd_code(uint8_t c) { return c == 'A' ? 0ull : c == 'C' ? 1ull : c == 'G' ? 2ull : 3ull; }
__device__ __forceinline__ char dd_letter(uint64_t x, int q) { return (char)(0x54474341u >> (8 * (int)((x >> (62 - 2 * q)) & 3))); }   // "ACGT"

// host ASCII in a staging buffer -> words: one thread per OUTPUT word packs its (up to) 32 letters; the bits behind them are 0
__global__ __launch_bounds__(256) void k_dd_pack(const uint8_t *__restrict__ ascii, const int64_t *__restrict__ boff, const int64_t *__restrict__ woff,
                                                 const int64_t *__restrict__ clen, int64_t n, int64_t total, uint64_t *__restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total) return;
    const int64_t c = pk_find(woff, n, w), j = w - woff[c];
    const int64_t cnt = clen[c] - 32 * j;
    const uint8_t *s = ascii + boff[c] + 32 * j;
    uint64_t x = 0;
#pragma unroll
    for (int q = 0; q < 32; q++) if (q < cnt) x |= dd_code(s[q]) << (62 - 2 * q);
    out[w] = x;
}
// words -> ASCII: one thread per word writes its (up to) 32 letters
__global__ __launch_bounds__(256) void k_dd_unpack(const uint64_t *__restrict__ words, const int64_t *__restrict__ woff, const int64_t *__restrict__ clen,
                                                   const int64_t *__restrict__ boff, int64_t n, int64_t total, uint8_t *__restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total) return;
    const int64_t c = pk_find(woff, n, w), j = w - woff[c];
    const int64_t cnt = clen[c] - 32 * j;
    const uint64_t x = words[w];
    uint8_t *d = out + boff[c] + 32 * j;
#pragma unroll
    for (int q = 0; q < 32; q++) if (q < cnt) d[q] = (uint8_t)dd_letter(x, q);
}

static int dd_alloc_meta(rfx_ctx *ctx, DdSet &d) {               // the device copies of h_woff / h_len
    RFX_ALLOC(d.woff, int64_t, d.n + 1);
    RFX_ALLOC(d.len, int64_t, std::max<int64_t>(d.n, 1));
    RFX_HIP(hipMemcpyAsync(d.woff.p, d.h_woff.data(), (size_t)(d.n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (d.n) RFX_HIP(hipMemcpyAsync(d.len.p, d.h_len.data(), (size_t)d.n * 8, hipMemcpyHostToDevice, ctx->stream));
    return RFX_OK;
}
// host ASCII + offsets -> a packed set in HBM (the library's own buffers): one upload, then one thread per output word
static int dd_pack_host(rfx_ctx *ctx, const uint8_t *bases, const int64_t *off, int64_t n, DdSet &d) {
    d.n = n;
    d.h_woff.assign((size_t)n + 1, 0); d.h_len.assign((size_t)n, 0);
    std::vector<int64_t> rel((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        const int64_t L = off[i + 1] - off[i];
        if (L < 0) { ctx->last_error = "contigs: offsets that run backwards"; return RFX_E_ARG; }
        d.h_len[(size_t)i] = L;
        d.h_woff[(size_t)i + 1] = d.h_woff[(size_t)i] + (L + 31) / 32;
        rel[(size_t)i + 1] = off[i + 1] - off[0];
    }
    d.words = d.h_woff[(size_t)n];
    const int64_t nb = rel[(size_t)n];
    RFX_ALLOC(d.w, uint64_t, std::max<int64_t>(d.words, 1));
    RFX_TRY(dd_alloc_meta(ctx, d));
    if (d.words > 0) {
        DevBuf stage, boff;
        RFX_HIP(stage.alloc((size_t)nb, ctx->stream)); RFX_ALLOC(boff, int64_t, n + 1);
        RFX_HIP(hipMemcpyAsync(stage.p, bases + off[0], (size_t)nb, hipMemcpyHostToDevice, ctx->stream));
        RFX_HIP(hipMemcpyAsync(boff.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        RFX_LAUNCH_N(k_dd_pack, d.words, stage.as<uint8_t>(), boff.as<int64_t>(),
                     d.woff.as<int64_t>(), d.len.as<int64_t>(), n, d.words, d.w.as<uint64_t>());
        RFX_TRY(sync_checked(ctx));                               // (`rel` and the staging buffers are read until here)
    }
    return sync_checked(ctx);
}
// a packed set -> host ASCII + offsets (the capacities were checked by the caller)
static int dd_unpack_host(rfx_ctx *ctx, const DdSet &d, uint8_t *out_bases, int64_t *out_off) {
    std::vector<int64_t> boff((size_t)d.n + 1, 0);
    for (int64_t i = 0; i < d.n; i++) boff[(size_t)i + 1] = boff[(size_t)i] + d.h_len[(size_t)i];
    const int64_t nb = boff[(size_t)d.n];
    for (int64_t i = 0; i <= d.n; i++) out_off[i] = boff[(size_t)i];
    if (nb == 0) return RFX_OK;
    DevBuf stage, d_boff;
    RFX_HIP(stage.alloc((size_t)nb, ctx->stream)); RFX_ALLOC(d_boff, int64_t, d.n + 1);
    RFX_HIP(hipMemcpyAsync(d_boff.p, boff.data(), (size_t)(d.n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    RFX_LAUNCH_N(k_dd_unpack, d.words, d.w.as<uint64_t>(), d.woff.as<int64_t>(),
                 d.len.as<int64_t>(), d_boff.as<int64_t>(), d.n, d.words, stage.as<uint8_t>());
    RFX_HIP(hipMemcpyAsync(out_bases, stage.p, (size_t)nb, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx);
}

// ---- the contig text the path writes, in HBM -> a packed set: sizes, a scan and a fill by output word ----------------------------
// A line that begins with '>' opens a contig; every other line behind the first header is that contig's bases, at any line
// width; '\r' is dropped; lines ahead of the first header are ignored; a header followed by a header or by the end is a contig
// of 0 bases that keeps its position (ids are positions).
// per byte: bit 0 = a line starts here, bit 32 = that line is a header; the scan of these gives every byte its line and the
// number of headers at or ahead of it
__global__ __launch_bounds__(256) void k_dd_text_starts(const char *__restrict__ t, int64_t len, uint64_t *__restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const bool ls = i == 0 || t[i - 1] == '\n';
    v[i] = ls ? (t[i] == '>' ? (1ull << 32) | 1ull : 1ull) : 0ull;
}
__global__ __launch_bounds__(256) void k_dd_text_lines(const char *__restrict__ t, int64_t len, const uint64_t *__restrict__ pv, uint8_t *__restrict__ hdrline,
                                                       int64_t *__restrict__ hpos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len || !(i == 0 || t[i - 1] == '\n')) return;
    const bool hs = t[i] == '>';
    hdrline[(uint32_t)pv[i]] = hs ? 1 : 0;
    if (hs) hpos[pv[i] >> 32] = i;
}
__global__ __launch_bounds__(256) void k_dd_text_isbase(const char *__restrict__ t, int64_t len, const uint64_t *__restrict__ pv, const uint8_t *__restrict__ hdrline,
                                                        uint32_t *__restrict__ isb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const uint64_t p = pv[i + 1];                                // (inclusive of byte i)
    const char c = t[i];
    isb[i] = ((p >> 32) >= 1 && !hdrline[(uint32_t)p - 1] && c != '\n' && c != '\r') ? 1u : 0u;
}
// gb = bases ahead of every byte: contig c holds the bases between its header and the next one
__global__ __launch_bounds__(256) void k_dd_text_sizes(const int64_t *__restrict__ hpos, int64_t n, const uint64_t *__restrict__ gb, int64_t len,
                                                       int64_t *__restrict__ clen, uint64_t *__restrict__ cw) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int64_t L = (int64_t)(gb[c + 1 < n ? hpos[c + 1] : len] - gb[hpos[c]]);
    clen[c] = L;
    cw[c] = (uint64_t)((L + 31) >> 5);
}
__global__ __launch_bounds__(256) void k_dd_text_fill(const char *__restrict__ t, int64_t len, const uint64_t *__restrict__ gb, const int64_t *__restrict__ hpos,
                                                      const int64_t *__restrict__ clen, const int64_t *__restrict__ woff, int64_t n, int64_t total,
                                                      uint64_t *__restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total) return;
    const int64_t c = pk_find(woff, n, w), j = w - woff[c];
    int64_t cnt = clen[c] - 32 * j;
    if (cnt > 32) cnt = 32;
    const uint64_t g = gb[hpos[c]] + (uint64_t)(32 * j);          // this word's first base, counted over the whole text
    int64_t lo = hpos[c], hi = len;                               // the last byte with gb <= g: that base
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (gb[mid] <= g) lo = mid; else hi = mid; }
    uint64_t x = 0;
    int k = 0;
    for (int64_t i = lo; k < cnt && i < len; i++) {               // (inside a contig every byte but '\n' and '\r' is a base)
        const char ch = t[i];
        if (ch == '\n' || ch == '\r') continue;
        x |= dd_code((uint8_t)ch) << (62 - 2 * k);
        k++;
    }
    out[w] = x;
}
static int dd_from_text(rfx_ctx *ctx, const char *d_text, int64_t len, DdSet &d) {
    d.n = 0; d.words = 0;
    d.h_woff.assign(1, 0); d.h_len.clear();
    if (len >= ((int64_t)1 << 32)) { ctx->last_error = "contig text: 2^32 bytes or more"; return RFX_E_LIMIT; }
    int64_t n = 0;
    DevBuf pv, hdrline, hpos, gb;
    if (len > 0) {
        DevBuf v;
        RFX_ALLOC(v, uint64_t, len); RFX_ALLOC(pv, uint64_t, len + 1);
        RFX_LAUNCH_N(k_dd_text_starts, len, d_text, len, v.as<uint64_t>());
        RFX_TRY(exclusive_scan_u64(ctx, v.as<uint64_t>(), pv.as<uint64_t>(), len));
        uint64_t tot = 0;
        RFX_TRY(small_readback(ctx, &tot, pv.as<uint64_t>() + len, 8));
        n = (int64_t)(tot >> 32);
        const int64_t nl = (int64_t)(uint32_t)tot;
        if (n > 0) {
            DevBuf isb;
            RFX_HIP(hdrline.alloc((size_t)nl, ctx->stream)); RFX_ALLOC(hpos, int64_t, n);
            RFX_ALLOC(isb, uint32_t, len); RFX_ALLOC(gb, uint64_t, len + 1);
            RFX_LAUNCH_N(k_dd_text_lines, len, d_text, len, pv.as<uint64_t>(), hdrline.as<uint8_t>(), hpos.as<int64_t>());
            RFX_LAUNCH_N(k_dd_text_isbase, len, d_text, len, pv.as<uint64_t>(), hdrline.as<uint8_t>(),
                         isb.as<uint32_t>());
            RFX_TRY(exclusive_scan_u32_to_u64(ctx, isb.as<uint32_t>(), gb.as<uint64_t>(), len));
        }
    }
    d.n = n;
    RFX_ALLOC(d.woff, uint64_t, n + 1);
    RFX_ALLOC(d.len, int64_t, std::max<int64_t>(n, 1));
    if (n == 0) {
        RFX_HIP(d.w.alloc(8, ctx->stream));
        RFX_HIP(hipMemsetAsync(d.woff.p, 0, 8, ctx->stream));
        return sync_checked(ctx);
    }
    DevBuf cw;
    RFX_ALLOC(cw, uint64_t, n);
    RFX_LAUNCH_N(k_dd_text_sizes, n, hpos.as<int64_t>(), n, gb.as<uint64_t>(), len, d.len.as<int64_t>(),
                 cw.as<uint64_t>());
    RFX_TRY(exclusive_scan_u64(ctx, cw.as<uint64_t>(), d.woff.as<uint64_t>(), n));
    d.h_woff.resize((size_t)n + 1); d.h_len.resize((size_t)n);
    RFX_HIP(hipMemcpyAsync(d.h_woff.data(), d.woff.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_HIP(hipMemcpyAsync(d.h_len.data(), d.len.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RFX_TRY(sync_checked(ctx));
    d.words = d.h_woff[(size_t)n];
    RFX_ALLOC(d.w, uint64_t, std::max<int64_t>(d.words, 1));
    if (d.words > 0) {
        RFX_LAUNCH_N(k_dd_text_fill, d.words, d_text, len, gb.as<uint64_t>(), hpos.as<int64_t>(),
                     d.len.as<int64_t>(), d.woff.as<int64_t>(), n, d.words, d.w.as<uint64_t>());
    }
    return sync_checked(ctx);
}

// ---- TagRowContigDSID.call + changeLine (:3397-3443): ">Contig-<len>-<idx>\n" + the sequence in lines of 10,000,000 bases, for
// the contigs of at least min_contig bases; idx = the position among ALL contigs of the set -------------------------------------
constexpr int64_t DD_LINE = 10000000;
__device__ __forceinline__ int dd_digits(int64_t v) { int c = 1; while (v >= 10) { v /= 10; c++; } return c; }
__device__ __forceinline__ int64_t dd_head_chars(int64_t L, int64_t i) { return 8 + dd_digits(L) + 1 + dd_digits(i) + 1; }
__global__ __launch_bounds__(256) void k_dd_out_sizes(const int64_t *__restrict__ clen, int64_t n, int64_t min_contig, uint64_t *__restrict__ sz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t L = clen[i], lines = (L + DD_LINE - 1) / DD_LINE;
    sz[i] = L < min_contig ? 0ull : (uint64_t)(dd_head_chars(L, i) + L + (lines > 1 ? lines : 1));
}
// one thread per contig: its header and its line ends.  Nothing at or past lim (the smaller of the text's length and the buffer)
__global__ __launch_bounds__(256) void k_dd_out_heads(const int64_t *__restrict__ clen, int64_t n, int64_t min_contig, const uint64_t *__restrict__ toff,
                                                      int64_t lim, char *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t L = clen[i];
    if (L < min_contig) return;
    int64_t p = (int64_t)toff[i];
    auto put = [&](char c) { if (p < lim) out[p] = c; p++; };
    auto number = [&](int64_t v) {
        int64_t top = 1;
        for (int c = dd_digits(v); c > 1; c--) top *= 10;
        for (; top > 0; top /= 10) put((char)('0' + (v / top) % 10));
    };
    put('>'); put('C'); put('o'); put('n'); put('t'); put('i'); put('g'); put('-');
    number(L); put('-'); number(i); put('\n');
    for (int64_t j0 = DD_LINE; j0 < L; j0 += DD_LINE) {           // the break ahead of base j0
        const int64_t q = p + j0 + j0 / DD_LINE - 1;
        if (q < lim) out[q] = '\n';
    }
    const int64_t last = (int64_t)toff[i + 1] - 1;
    if (last < lim) out[last] = '\n';
}
// one thread per word: its (up to) 32 letters
__global__ __launch_bounds__(256) void k_dd_out_bases(const uint64_t *__restrict__ words, const int64_t *__restrict__ woff, const int64_t *__restrict__ clen,
                                                      int64_t n, int64_t total, int64_t min_contig, const uint64_t *__restrict__ toff, int64_t lim,
                                                      char *__restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total) return;
    const int64_t c = pk_find(woff, n, w), j = w - woff[c], L = clen[c];
    if (L < min_contig) return;
    const int64_t cnt = L - 32 * j, b0 = 32 * j;
    int64_t line = b0 / DD_LINE, next = (line + 1) * DD_LINE;     // (a word may straddle a line break)
    const int64_t body = (int64_t)toff[c] + dd_head_chars(L, c);
    const uint64_t x = words[w];
#pragma unroll
    for (int q = 0; q < 32; q++) {
        if (q >= cnt) break;
        const int64_t b = b0 + q;
        if (b >= next) { line++; next += DD_LINE; }
        const int64_t p = body + b + line;
        if (p < lim) out[p] = dd_letter(x, q);
    }
}
// the text of a set into d_text (filled up to cap, nothing at or past it); *total = its length; own: a buffer of the library's,
// as long as the text
static int dd_to_text(rfx_ctx *ctx, const DdSet &d, int64_t min_contig, char *d_text, int64_t cap, int64_t *total, DevBuf *own) {
    const int64_t n = d.n;
    *total = 0;
    if (n == 0) return RFX_OK;
    DevBuf sz, toff;
    RFX_ALLOC(sz, uint64_t, n); RFX_ALLOC(toff, uint64_t, n + 1);
    RFX_LAUNCH_N(k_dd_out_sizes, n, d.len.as<int64_t>(), n, min_contig, sz.as<uint64_t>());
    RFX_TRY(exclusive_scan_u64(ctx, sz.as<uint64_t>(), toff.as<uint64_t>(), n));
    uint64_t t = 0;
    RFX_TRY(small_readback(ctx, &t, toff.as<uint64_t>() + n, 8));
    *total = (int64_t)t;
    if (own) {
        RFX_HIP(own->alloc((size_t)std::max<int64_t>(*total, 1), ctx->stream));
        d_text = own->as<char>(); cap = *total;
    }
    const int64_t lim = std::min<int64_t>(*total, cap);
    if (lim > 0) {
        RFX_LAUNCH_N(k_dd_out_heads, n, d.len.as<int64_t>(), n, min_contig, toff.as<uint64_t>(), lim, d_text);
        if (d.words > 0)
            RFX_LAUNCH_N(k_dd_out_bases, d.words, d.w.as<uint64_t>(), d.woff.as<int64_t>(),
                         d.len.as<int64_t>(), n, d.words, min_contig, toff.as<uint64_t>(), lim, d_text);
    }
    return sync_checked(ctx);
}

// ---- the caller's packed arrays (rfx_contigs_packed, device pointers) <-> DdSet ---------------------------------------------------
static bool dd_packed_out_ok(const rfx_contigs_packed *p) { return p && p->words && p->word_off && p->len; }
static bool dd_packed_ok(const rfx_contigs_packed *p) { return dd_packed_out_ok(p) && p->n >= 0; }
// a view of the caller's input set: nothing is copied in HBM, nothing is freed; the offsets and lengths come to the host, where
// the plan needs them, and are checked against the layout
static int dd_borrow(rfx_ctx *ctx, const rfx_contigs_packed *p, DdSet &d) {
    auto b = [&](DevBuf &x, void *q) { x.release(); x.p = q; x.s = ctx->stream; x.borrowed = true; };
    b(d.w, p->words); b(d.woff, p->word_off); b(d.len, p->len);
    const int64_t n = p->n;
    d.n = n;
    d.h_woff.assign((size_t)n + 1, 0); d.h_len.assign((size_t)n, 0);
    if (n > 0) {
        RFX_HIP(hipMemcpyAsync(d.h_woff.data(), p->word_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        RFX_HIP(hipMemcpyAsync(d.h_len.data(), p->len, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        RFX_TRY(sync_checked(ctx));
        if (d.h_woff[0] != 0) { ctx->last_error = "contigs: word_off[0] must be 0"; return RFX_E_ARG; }
        for (int64_t i = 0; i < n; i++)
            if (d.h_len[(size_t)i] < 0 || d.h_woff[(size_t)i + 1] - d.h_woff[(size_t)i] != (d.h_len[(size_t)i] + 31) / 32) {
                ctx->last_error = "contigs: word_off and len disagree (word_off[i+1] - word_off[i] = (len[i] + 31) / 32)";
                return RFX_E_ARG;
            }
    }
    d.words = d.h_woff[(size_t)n];
    return RFX_OK;
}
// the result into the caller's arrays; both capacities are checked before anything is copied
static int dd_store(rfx_ctx *ctx, const DdSet &d, rfx_contigs_packed *o) {
    const int64_t n = d.n, words = d.words;
    o->need_n = n; o->need_words = words;
    if (n > o->cap_n || words > o->cap_words) return RFX_E_CAP;
    o->n = n;
    if (words) RFX_HIP(hipMemcpyAsync(o->words, d.w.p, (size_t)words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    RFX_HIP(hipMemcpyAsync(o->word_off, d.h_woff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n) RFX_HIP(hipMemcpyAsync(o->len, d.h_len.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    return sync_checked(ctx);
}

struct Contig { int64_t woff, len, id; };     // a contig of the round's input pool (woff in words)
struct RowC { const uint64_t *w; int64_t len, id; };   // a row of the removal class: packed words in HBM
struct Row { int kind; int64_t id; int64_t idx; int64_t target; };   // kind 0: contig `idx` of the pool; 1: a marker row {-1, target}

// the three rounds: in (a packed set, its arrays in HBM and its offsets / lengths on the host) -> out (the library's own buffers)
static int dedup_run(rfx_ctx *ctx, const DdSet &in, DdSet &out, int64_t *round_n) {
    const int64_t n = in.n;
    std::vector<Contig> cur((size_t)n);
    for (int64_t i = 0; i < n; i++) cur[(size_t)i] = Contig{in.h_woff[(size_t)i], in.h_len[(size_t)i], i};
    // a round reads one pool and writes the next; round 1 reads the caller's words where they lie.  Everything is sized in
    // words: a merge of a and b bases needs ceil((a + b) / 32) <= ceil(a / 32) + ceil(b / 32) of them
    DevBuf pools[2];
    const uint64_t *pin = in.w.as<uint64_t>();
    int64_t used = in.words;

    for (int rnd = 1; rnd <= 3; rnd++) {
        const int both = rnd > 1;
        const int64_t nc = (int64_t)cur.size();
        // ---- markers
        std::vector<int64_t> coff((size_t)nc), clen((size_t)nc), cid((size_t)nc), moff((size_t)nc + 1, 0);
        for (int64_t i = 0; i < nc; i++) {
            coff[(size_t)i] = cur[(size_t)i].woff; clen[(size_t)i] = cur[(size_t)i].len; cid[(size_t)i] = cur[(size_t)i].id;
            moff[(size_t)i + 1] = moff[(size_t)i] + dd_seed_count(clen[(size_t)i]) + dd_probe_positions(clen[(size_t)i]) * (both ? 2 : 1);
        }
        const int64_t M = moff[(size_t)nc];
        if (M >= ((int64_t)1 << 32)) { ctx->last_error = "dedup: more than 2^32 marker rows"; return RFX_E_LIMIT; }
        std::vector<uint64_t> cand;                         // pair ids seen at least twice, ascending
        if (M > 0) {
            DevBuf d_meta, key, val, attr, tk, tv, pair, pk, pcnt, ck;
            RFX_ALLOC(d_meta, int64_t, 4 * nc + 1);
            int64_t *dm = d_meta.as<int64_t>();
            RFX_HIP(hipMemcpyAsync(dm, coff.data(), (size_t)nc * 8, hipMemcpyHostToDevice, ctx->stream));
            RFX_HIP(hipMemcpyAsync(dm + nc, clen.data(), (size_t)nc * 8, hipMemcpyHostToDevice, ctx->stream));
            RFX_HIP(hipMemcpyAsync(dm + 2 * nc, cid.data(), (size_t)nc * 8, hipMemcpyHostToDevice, ctx->stream));
            RFX_HIP(hipMemcpyAsync(dm + 3 * nc, moff.data(), (size_t)(nc + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            RFX_ALLOC(key, uint64_t, M); RFX_ALLOC(tk, uint64_t, M);
            RFX_ALLOC(val, uint32_t, M); RFX_ALLOC(tv, uint32_t, M);
            RFX_ALLOC(attr, int64_t, M); RFX_ALLOC(pair, int64_t, M);
            RFX_ALLOC(pk, uint64_t, M); RFX_ALLOC(ck, uint64_t, M);
            RFX_HIP(pcnt.alloc(16, ctx->stream));
            RFX_LAUNCH_N(k_dd_markers, M, pin, (const int64_t *)dm, (const int64_t *)(dm + nc), (const int64_t *)(dm + 2 * nc),
                         (const int64_t *)(dm + 3 * nc), nc, M, both, key.as<uint64_t>(), val.as<uint32_t>(), attr.as<int64_t>());
            RFX_TRY(sort_pairs(ctx, key.as<uint64_t>(), val.as<uint32_t>(), M, 64, tk.as<uint64_t>(), tv.as<uint32_t>()));
            RFX_LAUNCH_N(k_dd_select, M, key.as<uint64_t>(), val.as<uint32_t>(),
                         attr.as<int64_t>(), M, pair.as<int64_t>());
            RFX_HIP(hipMemsetAsync(pcnt.p, 0, 16, ctx->stream));
            RFX_LAUNCH_N(k_dd_compact_pairs, M, pair.as<int64_t>(), M, pk.as<uint64_t>(), pcnt.as<unsigned long long>());
            unsigned long long np = 0;
            RFX_HIP(hipMemcpyAsync(&np, pcnt.p, 8, hipMemcpyDeviceToHost, ctx->stream));
            RFX_TRY(sync_checked(ctx));
            if (np > 1) {
                RFX_TRY(sort_pairs(ctx, pk.as<uint64_t>(), val.as<uint32_t>(), (int64_t)np, 64, tk.as<uint64_t>(), tv.as<uint32_t>()));
                RFX_HIP(hipMemsetAsync(pcnt.p, 0, 16, ctx->stream));
                RFX_LAUNCH_N(k_dd_pair_runs, (int64_t)np, pk.as<uint64_t>(), (int64_t)np, ck.as<uint64_t>(),
                             pcnt.as<unsigned long long>());
                unsigned long long ncand = 0;
                RFX_HIP(hipMemcpyAsync(&ncand, pcnt.p, 8, hipMemcpyDeviceToHost, ctx->stream));
                RFX_TRY(sync_checked(ctx));
                cand.resize((size_t)ncand);
                if (ncand) RFX_HIP(hipMemcpyAsync(cand.data(), ck.p, (size_t)ncand * 8, hipMemcpyDeviceToHost, ctx->stream));
                RFX_TRY(sync_checked(ctx));
                std::sort(cand.begin(), cand.end());       // (the kernel appends in any order; groupBy().count() rows ascending)
            }
        }
        // ---- the plan: union, sort("count"), DSShorterRCContigSeqAndTargetExtraction (:3102-3131), sort("count") -- on ids
        std::vector<Row> u;
        for (int64_t i = 0; i < nc; i++) u.push_back(Row{0, cur[(size_t)i].id, i, 0});
        for (uint64_t p : cand) u.push_back(Row{1, (int64_t)(int32_t)(p >> 32), -1, (int64_t)(int32_t)p});      // DSMarkerKmerShorterID :3192-3199
        std::stable_sort(u.begin(), u.end(), [](const Row &a, const Row &b) { return a.id < b.id; });
        std::vector<Row> st;
        const Row *last = nullptr;
        for (size_t q = 0; q < u.size(); q++) {
            const Row *s = &u[q];
            if (!last) { last = s; continue; }
            if (s->id == last->id) {
                if (s->kind == 1) { Row r = *last; r.id = s->target; st.push_back(r); }
                else if (last->kind == 1) { Row r = *s; r.id = last->target; st.push_back(r); }
                last = nullptr;
            } else { st.push_back(*last); last = s; }
        }
        if (last) st.push_back(*last);
        std::stable_sort(st.begin(), st.end(), [](const Row &a, const Row &b) { return a.id < b.id; });
        // a leftover marker row {-1, target} is read as blocks by the removal class: 31 T's and the bases
        // currentKmerSizeFromBinaryBlockArray (:1636-1645) finds in `target` -- at most 62 bases, generated here as packed words
        // (two per row) and uploaded in one piece
        std::vector<RowC> rows;
        std::vector<uint64_t> mwords;
        std::vector<size_t> mrow;                                // the rows that live in mwords, two words apart
        for (const Row &r : st) {
            if (r.kind == 0) { rows.push_back(RowC{pin + cur[(size_t)r.idx].woff, cur[(size_t)r.idx].len, r.id}); continue; }
            const uint64_t t = (uint64_t)r.target;
            const int tz = t ? __builtin_ctzll(t) : 64;
            const int64_t len = std::max<int64_t>(0, 31 + (32 - tz / 2 - 1));
            uint64_t g[2] = {0, 0};
            for (int64_t i = 0; i < len; i++) {
                const uint64_t b = i < 31 ? 3 : (t >> (2 * (31 - (i - 31)))) & 3;
                g[i >> 5] |= b << (62 - 2 * (int)(i & 31));
            }
            mrow.push_back(rows.size());
            mwords.push_back(g[0]); mwords.push_back(g[1]);
            rows.push_back(RowC{nullptr, len, r.id});
        }
        DevBuf d_mrows;
        if (!mrow.empty()) {
            RFX_ALLOC(d_mrows, uint64_t, mwords.size());
            RFX_HIP(hipMemcpyAsync(d_mrows.p, mwords.data(), mwords.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            for (size_t q = 0; q < mrow.size(); q++) rows[mrow[q]].w = d_mrows.as<uint64_t>() + 2 * q;
        }
        // ---- the removal class (:1413-1460 / :516-563): groups of equal id, merged into their longest.  Step j of the round
        // merges the j-th short contig of EVERY group in one batch of launches (the groups are independent; inside a group
        // the shorts meet the growing long contig in row order, as in the reference's loop).
        const int variant = rnd == 1 ? 0 : 1;
        struct Group {
            size_t li; std::vector<size_t> shorts;
            const uint64_t *lng; int64_t ln;                  // the long contig as it stands
            int64_t woff, wcap;                               // the group's place in the two work buffers (words)
            std::vector<size_t> back;                         // shorts that found no place: back to the pool, ahead of the long one
        };
        std::vector<Group> groups;
        int64_t wused = 0;
        size_t max_shorts = 0;
        for (size_t g0 = 0; g0 < rows.size();) {
            size_t g1 = g0 + 1;
            while (g1 < rows.size() && rows[g1].id == rows[g0].id) g1++;
            Group G;
            G.li = g0;
            for (size_t q = g0 + 1; q < g1; q++) {            // the longest of the group (the first of the longest), the others in row order
                if (rows[q].len > rows[G.li].len) { G.shorts.push_back(G.li); G.li = q; } else G.shorts.push_back(q);
            }
            G.lng = rows[G.li].w; G.ln = rows[G.li].len; G.woff = wused; G.wcap = 0;
            if (!G.shorts.empty()) { for (size_t q = g0; q < g1; q++) G.wcap += (rows[q].len + 31) / 32; }
            wused += G.wcap;
            max_shorts = std::max(max_shorts, G.shorts.size());
            groups.push_back(std::move(G));
            g0 = g1;
        }
        DevBuf workA, workB;
        RFX_ALLOC(workA, uint64_t, std::max<int64_t>(wused, 1)); RFX_ALLOC(workB, uint64_t, std::max<int64_t>(wused, 1));
        uint64_t *const wa = workA.as<uint64_t>(), *const wb = workB.as<uint64_t>();
        DevBuf d_mb, d_eb, d_tkey, d_tpos, d_dist, d_dtmp, d_dval, d_dvtmp, d_cnt, d_seg, d_fd;
        RFX_HIP(d_cnt.alloc(16, ctx->stream));
        auto run_emits = [&](std::vector<EmitB> &eb) -> int {
            int64_t pre = 0;
            for (auto &e : eb) { e.pre = pre; pre += (e.a.n + e.b.n + 31) / 32; }
            if (eb.empty() || pre == 0) return RFX_OK;
            RFX_ALLOC(d_eb, EmitB, eb.size());
            RFX_HIP(hipMemcpyAsync(d_eb.p, eb.data(), eb.size() * sizeof(EmitB), hipMemcpyHostToDevice, ctx->stream));
            RFX_LAUNCH_N(k_dd_emit, pre, d_eb.as<EmitB>(), (int64_t)eb.size(), pre);
            RFX_TRY(sync_checked(ctx));                       // (`eb` is read by the queued copy until here)
            return RFX_OK;
        };
        for (size_t j = 0; j < max_shorts; j++) {
            std::vector<size_t> gi;                           // groups that have a j-th short
            for (size_t g = 0; g < groups.size(); g++) if (groups[g].shorts.size() > j) gi.push_back(g);
            const int64_t nm = (int64_t)gi.size();
            if (nm >= ((int64_t)1 << 30)) { ctx->last_error = "dedup: more than 2^30 merges in one step"; return RFX_E_LIMIT; }
            std::vector<MergeB> mb((size_t)nm);
            int64_t tslots = 0, sthreads = 0, qthreads = 0;
            for (int64_t m = 0; m < nm; m++) {
                Group &G = groups[gi[(size_t)m]];
                const size_t si = G.shorts[j];
                size_t want = 64;
                while (want < (size_t)(G.ln / 15 + 2) * 2 + 8) want *= 2;
                MergeB &M = mb[(size_t)m];
                M.lng = G.lng; M.ln = G.ln; M.sh = rows[si].w; M.sn = rows[si].len;
                M.toff = tslots; M.tmask = (uint32_t)want - 1;
                M.rc = variant == 1 ? 0 : 1; M.min_votes = variant == 0 ? 3 : 4; M.active = 1;     // variant 1: the forward strand first (:565-615)
                M.spre = sthreads; M.qpre = qthreads;
                tslots += (int64_t)want; sthreads += G.ln / 15 + 1; qthreads += std::max<int64_t>(M.sn, 1);
            }
            if (nm == 0) continue;
            RFX_ALLOC(d_mb, MergeB, nm);
            RFX_ALLOC(d_tkey, uint32_t, tslots); RFX_ALLOC(d_tpos, uint32_t, tslots);
            const size_t dcap = (size_t)qthreads * 2 + 16;    // (two query passes may append)
            RFX_ALLOC(d_dist, uint64_t, dcap); RFX_ALLOC(d_dtmp, uint64_t, dcap);
            RFX_ALLOC(d_dval, uint32_t, dcap); RFX_ALLOC(d_dvtmp, uint32_t, dcap);
            RFX_ALLOC(d_seg, int64_t, nm + 1); RFX_ALLOC(d_fd, int32_t, nm);
            RFX_HIP(hipMemcpyAsync(d_mb.p, mb.data(), (size_t)nm * sizeof(MergeB), hipMemcpyHostToDevice, ctx->stream));
            RFX_LAUNCH_N(k_dd_fill, tslots, d_tkey.as<uint32_t>(), DD_EMPTY, tslots);
            RFX_LAUNCH_N(k_dd_fill, tslots, d_tpos.as<uint32_t>(), 0xFFFFFFFFu, tslots);
            RFX_LAUNCH_N(k_dd_seed_insert_b, sthreads, d_mb.as<MergeB>(), nm, sthreads, d_tkey.as<uint32_t>(), d_tpos.as<int32_t>());
            RFX_HIP(hipMemsetAsync(d_cnt.p, 0, 16, ctx->stream));
            int key_bits = 33;
            while (((int64_t)1 << (key_bits - 33)) < nm) key_bits++;
            std::vector<int32_t> fd((size_t)nm, -1);
            // one query pass of the active merges + the vote on every active merge's (grown) list -> fd
            auto query_vote_b = [&]() -> int {
                RFX_LAUNCH_N(k_dd_query_b, qthreads, d_mb.as<MergeB>(), nm, qthreads, d_tkey.as<uint32_t>(),
                             d_tpos.as<int32_t>(), d_dist.as<uint64_t>(), d_cnt.as<unsigned long long>());
                unsigned long long c = 0;
                RFX_HIP(hipMemcpyAsync(&c, d_cnt.p, 8, hipMemcpyDeviceToHost, ctx->stream));
                RFX_TRY(sync_checked(ctx));
                // (a second pass appends to a SORTED prefix: the whole list is sorted again, as Collections.sort does)
                RFX_TRY(sort_pairs(ctx, d_dist.as<uint64_t>(), d_dval.as<uint32_t>(), (int64_t)c, key_bits, d_dtmp.as<uint64_t>(), d_dvtmp.as<uint32_t>()));
                RFX_LAUNCH_N(k_dd_seg_bounds, nm + 1, d_dist.as<uint64_t>(), (int64_t)c, nm, d_seg.as<int64_t>());
                RFX_LAUNCH(k_dd_vote, dim3((unsigned)nm), dim3(64), 0, d_dist.as<uint64_t>(),
                           d_seg.as<int64_t>(), d_mb.as<MergeB>(), (int64_t)0, 0, d_fd.as<int32_t>());
                std::vector<int32_t> got((size_t)nm);
                RFX_HIP(hipMemcpyAsync(got.data(), d_fd.p, (size_t)nm * 4, hipMemcpyDeviceToHost, ctx->stream));
                RFX_TRY(sync_checked(ctx));
                for (int64_t m = 0; m < nm; m++) if (mb[(size_t)m].active) fd[(size_t)m] = got[(size_t)m];
                return RFX_OK;
            };
            std::vector<EmitB> eb;
            std::vector<char> done((size_t)nm, 0);
            // what a vote means for merge m (rc: the strand the short contig was read in): a merged contig is ONE descriptor of
            // two pieces, written into the group's place in the work buffer the long contig does not lie in
            auto apply = [&](int64_t m, int rc, bool last_pass) {
                Group &G = groups[gi[(size_t)m]];
                const size_t si = G.shorts[j];
                const uint64_t *sh = rows[si].w;
                const int64_t sn = rows[si].len, ln = G.ln;
                const int32_t f = fd[(size_t)m];
                uint64_t *dst = (G.lng == wa + G.woff ? wb : wa) + G.woff;
                if (f == -1) { if (last_pass) { G.back.push_back(si); done[(size_t)m] = 1; } return; }      // (:1499-1503: back to the pool)
                if (f == 0) { if (last_pass) done[(size_t)m] = 1; return; }
                if (f < 0) {
                    int64_t flank = sn - (ln + f);
                    if (flank > sn) flank = sn;
                    if (flank > 0) {
                        eb.push_back(EmitB{dst, DdSeg{G.lng, ln, 0, ln, 0, 0}, DdSeg{sh, sn, sn - flank, flank, rc, 0}, 0});
                        G.lng = dst; G.ln = ln + flank; done[(size_t)m] = 1;
                    } else if (last_pass) done[(size_t)m] = 1;
                } else {
                    const int64_t p = std::min<int64_t>(sn, f);
                    eb.push_back(EmitB{dst, DdSeg{sh, sn, 0, p, rc, 0}, DdSeg{G.lng, ln, 0, ln, 0, 0}, 0});
                    G.lng = dst; G.ln = ln + p; done[(size_t)m] = 1;
                }
            };
            RFX_TRY(query_vote_b());
            if (variant == 1) {
                for (int64_t m = 0; m < nm; m++) apply(m, 0, false);
                // the merges the forward strand did not settle go on to the reverse complement (:616-728), their list growing
                bool any = false;
                for (int64_t m = 0; m < nm; m++) { mb[(size_t)m].active = done[(size_t)m] ? 0 : 1; mb[(size_t)m].rc = 1; mb[(size_t)m].min_votes = 4; any = any || !done[(size_t)m]; }
                if (any) {
                    RFX_HIP(hipMemcpyAsync(d_mb.p, mb.data(), (size_t)nm * sizeof(MergeB), hipMemcpyHostToDevice, ctx->stream));
                    RFX_TRY(query_vote_b());
                    for (int64_t m = 0; m < nm; m++) if (mb[(size_t)m].active) apply(m, 1, true);
                }
            } else {
                for (int64_t m = 0; m < nm; m++) apply(m, 1, true);
            }
            for (int64_t m = 0; m < nm; m++) {
                const Group &G = groups[gi[(size_t)m]];
                if ((G.ln + 31) / 32 > G.wcap) { ctx->last_error = "dedup: a merged contig outgrew its work area"; return RFX_E_LIMIT; }
            }
            RFX_TRY(run_emits(eb));
        }
        // ---- the round's output, in the reference's order: per group the shorts that went back to the pool, then the long one;
        // contig after contig, each on a word: the same kernel with "copy" descriptors
        std::vector<Contig> nxt;
        std::vector<EmitB> eb;
        int64_t out_words = 0;
        auto emit = [&](const uint64_t *src, int64_t len) {
            if (len) eb.push_back(EmitB{nullptr, DdSeg{src, len, 0, len, 0, 0}, DdSeg{nullptr, 0, 0, 0, 0, 0}, out_words});     // (pre: its place, until the pool exists)
            nxt.push_back(Contig{out_words, len, (int64_t)nxt.size()});
            out_words += (len + 31) / 32;
        };
        for (Group &G : groups) {
            for (size_t si : G.back) emit(rows[si].w, rows[si].len);
            emit(G.lng, G.ln);
        }
        DevBuf &pool = pools[rnd & 1];                        // (round 3 takes the slot of round 1's output, which nobody reads any more)
        RFX_ALLOC(pool, uint64_t, std::max<int64_t>(out_words, 1));
        for (auto &e : eb) e.dst = pool.as<uint64_t>() + e.pre;
        RFX_TRY(run_emits(eb));
        RFX_TRY(sync_checked(ctx));
        cur = nxt;                                              // zipWithIndex: ids = positions
        if (round_n) round_n[rnd - 1] = (int64_t)cur.size();
        pin = pool.as<uint64_t>();
        used = out_words;
    }
    out.n = (int64_t)cur.size();
    out.words = used;
    out.h_woff.assign(cur.size() + 1, 0); out.h_len.assign(cur.size(), 0);
    for (size_t i = 0; i < cur.size(); i++) { out.h_woff[i] = cur[i].woff; out.h_len[i] = cur[i].len; }
    out.h_woff[cur.size()] = used;
    out.w = std::move(pools[1]);
    RFX_TRY(dd_alloc_meta(ctx, out));
    return sync_checked(ctx);
}

}  // namespace

extern "C" {

// ---- the packed set in the caller's device arrays ------------------------------------------------------------------------------
int rfx_dev_contigs_pack(rfx_ctx *ctx, const uint8_t *bases_ascii, const int64_t *contig_off, int64_t n, rfx_contigs_packed *d_out) try {
    if (!ctx || !contig_off || n < 0 || !dd_packed_out_ok(d_out)) return RFX_E_ARG;
    if (n > 0 && contig_off[n] > contig_off[0] && !bases_ascii) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DdSet a;
    RFX_TRY(dd_pack_host(ctx, bases_ascii, contig_off, n, a));
    return dd_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_contigs_unpack(rfx_ctx *ctx, const rfx_contigs_packed *d_in, uint8_t *out_bases_ascii, int64_t cap_bases, int64_t *out_off,
                           int64_t cap_contigs, int64_t *out_n) try {
    if (!ctx || !dd_packed_ok(d_in) || !out_off || !out_n || cap_bases < 0 || cap_contigs < 0 || (cap_bases > 0 && !out_bases_ascii)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DdSet a;
    RFX_TRY(dd_borrow(ctx, d_in, a));
    int64_t nb = 0;
    for (int64_t L : a.h_len) nb += L;
    *out_n = a.n;
    if (nb > cap_bases || a.n > cap_contigs) { ctx->last_error = "contigs: needs room for " + std::to_string(nb) + " bases"; return RFX_E_CAP; }
    return dd_unpack_host(ctx, a, out_bases_ascii, out_off);
} RFX_API_CATCH(ctx)

int rfx_dev_contigs_from_text(rfx_ctx *ctx, const char *d_text, int64_t len, rfx_contigs_packed *d_out) try {
    if (!ctx || len < 0 || (len > 0 && !d_text) || !dd_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DdSet a;
    RFX_TRY(dd_from_text(ctx, d_text, len, a));
    return dd_store(ctx, a, d_out);
} RFX_API_CATCH(ctx)

int rfx_dev_contigs_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, int min_contig, char *d_text, int64_t cap, int64_t *out_len,
                            int64_t *out_contigs) try {
    if (!ctx || !dd_packed_ok(d_in) || !out_len || cap < 0 || (cap > 0 && !d_text)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DdSet a;
    int64_t total = 0, written = 0;
    RFX_TRY(dd_borrow(ctx, d_in, a));
    RFX_TRY(dd_to_text(ctx, a, min_contig, d_text, cap, &total, nullptr));
    for (int64_t L : a.h_len) written += L >= min_contig ? 1 : 0;
    *out_len = total;
    if (out_contigs) *out_contigs = written;
    return total > cap ? RFX_E_CAP : RFX_OK;
} RFX_API_CATCH(ctx)

int rfx_dev_dedup_contigs(rfx_ctx *ctx, const rfx_contigs_packed *d_in, rfx_contigs_packed *d_out, int64_t *round_n) try {
    if (!ctx || !dd_packed_ok(d_in) || !dd_packed_out_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DdSet a, b;
    RFX_TRY(dd_borrow(ctx, d_in, a));
    RFX_TRY(dedup_run(ctx, a, b, round_n));
    return dd_store(ctx, b, d_out);
} RFX_API_CATCH(ctx)

// ---- the host forms: pack (or from-text) -> the same kernels -> unpack / to-text -------------------------------------------------
// the text of the survivors into the caller's HOST buffer (text-buffer rule: filled up to cap, nothing at or past it)
static int dd_text_to_host(rfx_ctx *ctx, const DdSet &d, int min_contig, char *text, int64_t cap, int64_t *text_len) {
    DevBuf d_text;
    int64_t total = 0;
    RFX_TRY(dd_to_text(ctx, d, min_contig, nullptr, 0, &total, &d_text));
    *text_len = total;
    const int64_t lim = text ? std::min<int64_t>(total, cap) : 0;
    if (lim > 0) RFX_HIP(hipMemcpyAsync(text, d_text.p, (size_t)lim, hipMemcpyDeviceToHost, ctx->stream));
    RFX_TRY(sync_checked(ctx));
    return text && total > cap ? RFX_E_CAP : RFX_OK;
}

int rfx_dedup_contigs(rfx_ctx *ctx, const uint8_t *bases_ascii, const int64_t *contig_off, int64_t n_contigs, int min_contig,
                      uint8_t *out_bases_ascii, int64_t cap_bases, int64_t *out_off, int64_t cap_contigs, int64_t *out_n,
                      char *text, int64_t text_cap, int64_t *text_len, int64_t *round_n) try {
    if (!ctx || !contig_off || n_contigs < 0 || (n_contigs > 0 && !bases_ascii)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DdSet a, b;
    RFX_TRY(dd_pack_host(ctx, bases_ascii, contig_off, n_contigs, a));
    RFX_TRY(dedup_run(ctx, a, b, round_n));
    if (out_n) *out_n = b.n;
    int st = RFX_OK;
    if (out_bases_ascii && out_off) {
        int64_t nb = 0;
        for (int64_t L : b.h_len) nb += L;
        if (nb > cap_bases || b.n > cap_contigs) st = RFX_E_CAP;
        else RFX_TRY(dd_unpack_host(ctx, b, out_bases_ascii, out_off));
    }
    if (text_len) {
        const int ts = dd_text_to_host(ctx, b, min_contig, text, text_cap, text_len);
        if (ts != RFX_OK && ts != RFX_E_CAP) return ts;
        if (ts == RFX_E_CAP) st = RFX_E_CAP;
    }
    return st;
} RFX_API_CATCH(ctx)

// The same from the contig TEXT the path writes (">Contig-<len>-...\n" + the sequence wrapped at 100 columns; either twin's
// header): every record is a contig, in order, ids = positions -> the de-duplicated text (TagRowContigDSID's format).  The text
// is uploaded once; from-text, the rounds and to-text run on the packed set in HBM; one copy back.
int rfx_dedup_contig_text(rfx_ctx *ctx, const char *contig_text, int64_t len, int min_contig, char *out, int64_t cap, int64_t *out_len,
                          int64_t *out_contigs, int64_t *round_n) try {
    if (!ctx || (len > 0 && !contig_text) || !out_len) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_text;
    DdSet a, b;
    if (len > 0) {
        RFX_HIP(d_text.alloc((size_t)len, ctx->stream));
        RFX_HIP(hipMemcpyAsync(d_text.p, contig_text, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
    }
    RFX_TRY(dd_from_text(ctx, d_text.as<char>(), std::max<int64_t>(len, 0), a));
    RFX_TRY(dedup_run(ctx, a, b, round_n));
    if (out_contigs) *out_contigs = b.n;
    return dd_text_to_host(ctx, b, min_contig, out, cap, out_len);
} RFX_API_CATCH(ctx)

}  // extern "C"
