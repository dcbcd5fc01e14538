// rfx_endext.hip -- the end extension of contigs from alignment rows (Assembly_intermediate/07EndExtend) on packed sets that stay in
// HBM: P/ReflexivDSDynamicKmerMapping.java behind its aligner, driver :305-347 -- SAMString2ROW (:369-388),
// DSProcessSAMandExtendContigs (:564-994), the union with 05FixingAgain and sort("ID") (:320-331), DSExtendContigs (:413-562),
// zipWithIndex + TagStringContigRDDID (:1268-1286).  All alignment rows form ONE logical partition (the stated deviation), so the
// stage takes no P.  Nothing here is rfx_dynamic.hip's:
//   parse        one thread per row "name \t start \t cigar \t seq": the contig and the side out of the name (checked against the
//                input set), the start, one walk over the CIGAR, the marker test ahead of both -- into a fixed record: contig, left
//                source and count, right source and count, repeat bits.  No arrays
//   group        a key sort of the row numbers on the contig, one search per contig for its first row
//   pile-up      one workgroup per contig, both [300][4] tables in LDS, a wave per row and a lane per contributed base (LDS atomic
//                adds), then one lane per position for the argmax (a tie to the higher code) and one per output word
//   order        the ID's four decimal fields as 4-bit characters in three words ('-' < '0'..'9' < '_', 0 ends the text), sorted
//                with sort_columns: the byte order of the ID strings without a string
//   splice       ONE THREAD PER OUTPUT WORD: reversed left || contig || right, three segments through pk_seg32 / pk_rev2, masked at
//                the end (pk_keep).  Bases only: the literals "-1l" / "r1-" of a flagged side live in `flags`
//   text         as k_fx2_text_fill: sizes, a scan, one read-back, one thread per 16-byte chunk cut at the destination ADDRESS
#include <algorithm>
#include "rfx_internal.h"
#include "rfx_packed_words.h"
#include "rfx_endext_hits.h"

using namespace rfx;

namespace {

#define EE_LONGEST 300               // longestExtend (:567): positions of a consensus
#define EE_NEAR 10                   // a start / a tail of 10 or more skips the row (:685, :753)
#define EE_END 200                   // refLength of a -R row (:751)
#define EE_CW 10                     // words of a consensus
#define EE_WAVES 4                   // waves of the pile-up's workgroup

// what is wrong with a call's input (CallFlags::bad)
enum { EE_BAD_CIGAR = 1, EE_BAD_START = 2, EE_BAD_RANGE = 4, EE_BAD_LAYOUT = 8, EE_TOO_LONG = 16, EE_BAD_ID = 32, EE_BAD_HIT = 64 };

// what a row adds: lcnt bases read DOWN from text[lsrc] to the left table from j = 0, rcnt bases read UP from text[rsrc] to the right one
struct EeRow { int64_t lsrc, rsrc; int32_t contig, lcnt, rcnt; uint32_t rep; };

// char2int (:955-977): a/A 0, c/C 1, g/G 2, everything else 3
__device__ __forceinline__ uint32_t ee_code(char ch) {
    const char u = (char)(ch & 0xDF);
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : 3u;
}
// "Contig_<L>_<left>_<right>_<idx>" at t[p, e), p left behind it
__device__ __forceinline__ bool ee_id(const char *__restrict__ t, int64_t &p, int64_t e, int *L, int *left, int *right, int *idx) {
    if (e - p < 7) return false;
    bool ok = t[p] == 'C' && t[p + 1] == 'o' && t[p + 2] == 'n' && t[p + 3] == 't' && t[p + 4] == 'i' && t[p + 5] == 'g' && t[p + 6] == '_';
    p += 7;
    ok = ok && pk_dec_int(t, p, e, false, false, true, L) && p < e && t[p] == '_';
    p++;
    ok = ok && pk_dec_int(t, p, e, true, false, true, left) && p < e && t[p] == '_';
    p++;
    ok = ok && pk_dec_int(t, p, e, true, false, true, right) && p < e && t[p] == '_';
    p++;
    return ok && pk_dec_int(t, p, e, false, false, true, idx);
}

// ---- parse: SAMString2ROW (:369-388) and the per-row half of DSProcessSAMandExtendContigs (:668-869) -------------------------------
__global__ __launch_bounds__(256) void k_ee_parse(const char *__restrict__ text, const int64_t *__restrict__ row_off, int64_t n_rows,
                                                  const int64_t *__restrict__ len, const int32_t *__restrict__ left, const int32_t *__restrict__ right,
                                                  int64_t n, EeRow *__restrict__ rows, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                  CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t b = row_off[i];
    int64_t e = row_off[i + 1];
    while (e > b && (text[e - 1] == '\n' || text[e - 1] == '\r')) e--;
    EeRow r{0, 0, -1, 0, 0, 0u};
    // the first four fields; split("\t") drops trailing empty fields, so four fields are a third tab with anything but tabs behind it
    int64_t t1 = e, t2 = e, t3 = e, t4 = e;
    int tabs = 0;
    for (int64_t p = b; p < e && tabs < 4; p++) {
        if (text[p] == '\t') {
            tabs++;
            if (tabs == 1) t1 = p; else if (tabs == 2) t2 = p; else if (tabs == 3) t3 = p; else t4 = p;
        }
    }
    bool four = false;
    for (int64_t p = t3 + 1; p < e && !four; p++) four = text[p] != '\t';
    const int64_t s3 = t3 + 1, seqlen = four ? t4 - s3 : 0;
    // the name: the ID of the contig at its <idx>, with -L, -R or nothing behind it; any other row is ignored
    int L = 0, lf = 0, rt = 0, idx = 0, side = 0;
    int64_t p = b;
    bool ok = four && ee_id(text, p, t1, &L, &lf, &rt, &idx);
    if (ok && p != t1) {
        ok = t1 - p == 2 && text[p] == '-' && (text[p + 1] == 'L' || text[p + 1] == 'R');
        side = ok && text[p + 1] == 'L' ? 1 : 2;
    }
    ok = ok && idx < n && len[idx] == (int64_t)L && left[idx] == lf && right[idx] == rt;
    if (ok) {
        r.contig = idx;
        // the repeat markers of the script, ahead of any parsing (:678, :717, :777-791)
        const bool isL = seqlen == 1 && text[s3] == 'L', isR = seqlen == 1 && text[s3] == 'R';
        const bool isLR = seqlen == 3 && text[s3] == 'L' && text[s3 + 1] == '-' && text[s3 + 2] == 'R';
        r.rep = side == 1 ? (isL ? 1u : 0u) : side == 2 ? (isR ? 2u : 0u) : (isL ? 1u : isR ? 2u : isLR ? 3u : 0u);
    }
    if (ok && !r.rep) {
        uint32_t bad = 0;
        int start = 0;
        p = t1 + 1;
        if (!pk_dec_int(text, p, t2, true, true, false, &start) || p != t2) bad |= EE_BAD_START;
        // one walk over the CIGAR ([0-9]+[A-Z=])+: the first and the last operation, and the sum from the first M (from the first
        // operation where there is no M) up to the operation ahead of the last, I subtracting (:734-749).  An operation is added
        // when the next one is read, so the last never is
        int64_t c = t2 + 1, first_len = 0, pend_len = 0, sum_all = 0, sum_m = 0;
        char first_op = 0, pend_op = 0;
        bool seen_m = false, cig = c < t3;
        int nops = 0;
        while (cig && c < t3) {
            int64_t v = 0;
            int nd = 0;
            while (c < t3 && text[c] >= '0' && text[c] <= '9') { if (nd < 10) v = v * 10 + (text[c] - '0'); nd++; c++; }
            if (nd == 0 || nd > 9 || c >= t3) { cig = false; break; }
            const char op = text[c++];
            if (!((op >= 'A' && op <= 'Z') || op == '=')) { cig = false; break; }
            if (nops > 0) {
                if (pend_op == 'M') seen_m = true;
                const int64_t d = pend_op == 'I' ? -pend_len : pend_len;
                sum_all += d;
                if (seen_m) sum_m += d;
            } else {
                first_len = v; first_op = op;
            }
            pend_len = v; pend_op = op; nops++;
        }
        if (!cig) bad |= EE_BAD_CIGAR;
        if (!bad) {
            const int64_t align = seen_m ? sum_m : sum_all;
            // left (:683-713, :801-821): seq[o], seq[o - 1], ..., seq[0] -- o + 1 bases -- to j = 0, 1, ...
            if (side != 2 && first_op == 'S' && start < EE_NEAR) {
                const int64_t o = first_len - start;
                if (o > 0) {
                    if (o >= seqlen) bad |= EE_BAD_RANGE;
                    else { r.lsrc = s3 + o; r.lcnt = (int32_t)(o + 1 < EE_LONGEST ? o + 1 : EE_LONGEST); }
                }
            }
            // right (:726-772, :823-867): the last o bases of seq to j = 0, 1, ... in read order
            if (side != 1 && pend_op == 'S') {
                const int64_t ref = side == 2 ? EE_END : L, tail = ref - (align + start - 1);
                if (tail < EE_NEAR) {
                    const int64_t o = pend_len - tail;
                    if (o > 0) {
                        if (o > seqlen) bad |= EE_BAD_RANGE;
                        else { r.rsrc = s3 + seqlen - o; r.rcnt = (int32_t)(o < EE_LONGEST ? o : EE_LONGEST); }
                    }
                }
            }
        }
        if (bad) { atomicOr(&flags->bad, bad); r.lcnt = 0; r.rcnt = 0; }
    }
    rows[i] = r;
    keys[i] = r.contig >= 0 ? (uint64_t)r.contig : (uint64_t)n;     // (the ignored rows behind every contig's)
    vals[i] = (uint32_t)i;
}
// per contig c (and c = n): the first of the sorted rows whose key is c or more
__global__ __launch_bounds__(256) void k_ee_first(const uint64_t *__restrict__ keys, int64_t n_rows, int64_t n, int64_t *__restrict__ first) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n) return;
    int64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < (uint64_t)c) lo = mid + 1; else hi = mid;
    }
    first[c] = lo;
}

// ---- pile-up and consensus (:597-655, :883-949): one workgroup per contig ----------------------------------------------------------
// the tail of a pile-up's workgroup, behind the barrier that ends the counting: the argmax of every position, then the two consensus
// sequences, their lengths and the flags of contig c
__device__ __forceinline__ void ee_pile_finish(const uint32_t *tab, const uint32_t *rep, uint32_t *cnt, uint8_t *best, int64_t c, int tid,
                                               uint64_t *__restrict__ cons, int32_t *__restrict__ clen, int32_t *__restrict__ cflags) {
    for (int t = tid; t < 2 * EE_LONGEST; t += 64 * EE_WAVES) {       // a lane per position: the highest count, a tie to the HIGHER code
        uint32_t hi = 0u;
        int code = -1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t v = tab[4 * t + k];
            if (v != 0u && v >= hi) { hi = v; code = k; }
        }
        best[t] = (uint8_t)code;
        if (code >= 0) atomicAdd(&cnt[t >= EE_LONGEST ? 1 : 0], 1u);  // (every row covers a prefix of j: no holes)
    }
    __syncthreads();
    if (tid < 2 * EE_CW) {                                           // a lane per word of the two consensus sequences
        const int side = tid / EE_CW, w = tid % EE_CW, L = (int)cnt[side];
        uint64_t x = 0ull;
        for (int j = 0; j < 32; j++) {
            const int pos = 32 * w + j;
            if (pos < L) x |= pk_at((uint64_t)(best[side * EE_LONGEST + pos] & 3u), j);
        }
        cons[(c * 2 + side) * EE_CW + w] = x;
    }
    if (tid == 0) {
        clen[2 * c] = (int32_t)cnt[0]; clen[2 * c + 1] = (int32_t)cnt[1];
        cflags[c] = (rep[0] >= 2u ? 1 : 0) | (rep[1] >= 2u ? 2 : 0);
    }
}
__global__ __launch_bounds__(64 * EE_WAVES) void k_ee_pile(const char *__restrict__ text, const EeRow *__restrict__ rows, const uint32_t *__restrict__ order,
                                                           const int64_t *__restrict__ first, uint64_t *__restrict__ cons /* [n][2][EE_CW] */,
                                                           int32_t *__restrict__ clen /* [n][2] */, int32_t *__restrict__ cflags) {
    __shared__ uint32_t tab[2 * EE_LONGEST * 4];
    __shared__ uint32_t rep[2], cnt[2];
    __shared__ uint8_t best[2 * EE_LONGEST];
    const int64_t c = blockIdx.x;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int t = tid; t < 2 * EE_LONGEST * 4; t += 64 * EE_WAVES) tab[t] = 0u;
    if (tid < 2) { rep[tid] = 0u; cnt[tid] = 0u; }
    __syncthreads();
    const int64_t r1 = first[c + 1];
    for (int64_t q = first[c] + wave; q < r1; q += EE_WAVES) {        // a wave per row, so any row count works
        const EeRow r = rows[order[q]];
        if (lane == 0 && (r.rep & 1u)) atomicAdd(&rep[0], 1u);
        if (lane == 0 && (r.rep & 2u)) atomicAdd(&rep[1], 1u);
        for (int t = lane; t < r.lcnt + r.rcnt; t += 64) {            // a lane per contributed base
            const bool right = t >= r.lcnt;
            const int j = right ? t - r.lcnt : t;
            const char ch = right ? text[r.rsrc + j] : text[r.lsrc - j];
            atomicAdd(&tab[((right ? EE_LONGEST : 0) + j) * 4 + ee_code(ch)], 1u);
        }
    }
    __syncthreads();
    ee_pile_finish(tab, rep, cnt, best, c, tid, cons, clen, cflags);
}
// ---- the same pile-up from the hits of the end mapping, no row text (rfx_dev_endext_consensus_hits) ---------------------------------------
// one thread per hit: checked as rfx_dev_map_to_text checks it (mp_row, rfx_endmap.hip) BEFORE anything indexes with it, then what
// k_ee_parse would read out of its row (rfx_endext_hits.h).  The mapper writes no repeat-marker rows: rep stays 0
struct EhHit { int64_t read; int32_t contig, n, strand, lsrc, lcnt, rsrc, rcnt; };
__global__ __launch_bounds__(256) void k_eh_rows(const Fx2View c, const uint32_t *__restrict__ read_len, int wpr, const MpHits h, int64_t n_hits, int seed,
                                                 EhHit *__restrict__ rows, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, CallFlags *__restrict__ flags) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_hits) return;
    const int end = h.end[q], strand = h.strand[q], off = h.off[q], v = h.v[q];
    const int64_t read = h.read[q];
    EhHit r{0, -1, 0, 0, 0, 0, 0, 0};
    uint32_t bad = 0u;
    bool ok = end >= 0 && (int64_t)end < 2 * c.n && !(strand & ~1) && read >= 0;
    if (ok) {
        const int64_t ci = end >> 1, L64 = c.len[ci];
        ok = L64 >= seed && L64 < ((int64_t)1 << 30) && c.woff[ci + 1] - c.woff[ci] == ((L64 + 31) >> 5);
        const uint32_t n32 = ok ? read_len[read] : 0u;
        ok = ok && n32 <= 32u * (uint32_t)wpr;
        EhRow row;
        if (ok && eh_row(end & 1, (int)L64, (int)n32, off, v, seed, &row)) {
            const EhAdd a = eh_add(row, (int)n32, (int)L64);
            if (a.bad) bad = a.bad == 1 ? (uint32_t)EE_BAD_CIGAR : (uint32_t)EE_BAD_RANGE;
            r = EhHit{read, (int32_t)ci, (int32_t)n32, strand, a.lsrc, a.lcnt, a.rsrc, a.rcnt};
        } else {
            ok = false;
        }
    }
    if (!ok) bad = (uint32_t)EE_BAD_HIT;
    if (bad) atomicOr(&flags->bad, bad);
    rows[q] = r;
    keys[q] = r.contig >= 0 ? (uint64_t)r.contig : (uint64_t)c.n;
    vals[q] = (uint32_t)q;
}
// one workgroup per contig, both tables in LDS, a wave per hit and a lane per contributed base, as k_ee_pile; the base comes out of the
// 2-bit read store: position t of the orientation that matched is base t of the read, or the complement of its base n - 1 - t
__global__ __launch_bounds__(64 * EE_WAVES) void k_eh_pile(const uint64_t *__restrict__ words, int wpr, const EhHit *__restrict__ rows,
                                                           const uint32_t *__restrict__ order, const int64_t *__restrict__ first,
                                                           uint64_t *__restrict__ cons /* [n][2][EE_CW] */, int32_t *__restrict__ clen /* [n][2] */,
                                                           int32_t *__restrict__ cflags) {
    __shared__ uint32_t tab[2 * EE_LONGEST * 4];
    __shared__ uint32_t rep[2], cnt[2];
    __shared__ uint8_t best[2 * EE_LONGEST];
    const int64_t c = blockIdx.x;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int t = tid; t < 2 * EE_LONGEST * 4; t += 64 * EE_WAVES) tab[t] = 0u;
    if (tid < 2) { rep[tid] = 0u; cnt[tid] = 0u; }
    __syncthreads();
    const int64_t r1 = first[c + 1];
    for (int64_t q = first[c] + wave; q < r1; q += EE_WAVES) {
        const EhHit r = rows[order[q]];
        const uint64_t *rw = words + r.read * wpr;
        for (int t = lane; t < r.lcnt + r.rcnt; t += 64) {
            const bool right = t >= r.lcnt;
            const int j = right ? t - r.lcnt : t;
            const int pos = right ? r.rsrc + j : r.lsrc - j;
            const uint32_t code = r.strand ? 3u - pk_base_of(rw, r.n - 1 - pos) : pk_base_of(rw, pos);
            atomicAdd(&tab[((right ? EE_LONGEST : 0) + j) * 4 + code], 1u);
        }
    }
    __syncthreads();
    ee_pile_finish(tab, rep, cnt, best, c, tid, cons, clen, cflags);
}
__global__ __launch_bounds__(256) void k_ee_cons_sizes(const int32_t *__restrict__ clen, int64_t n, uint32_t *__restrict__ nwl, uint32_t *__restrict__ nwr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    nwl[i] = (uint32_t)((clen[2 * i] + 31) >> 5);
    nwr[i] = (uint32_t)((clen[2 * i + 1] + 31) >> 5);
}
// threads [0, n): a contig's fields in both sets; threads [n, n + 2 EE_CW n): one word of the scratch each, where the consensus has it
__global__ __launch_bounds__(256) void k_ee_cons_emit(const uint64_t *__restrict__ cons, const int32_t *__restrict__ clen, const int32_t *__restrict__ cflags,
                                                      const uint64_t *__restrict__ offl, const uint64_t *__restrict__ offr, int64_t n, uint64_t *__restrict__ lw,
                                                      int64_t *__restrict__ lwoff, int64_t *__restrict__ llen, uint64_t *__restrict__ rw, int64_t *__restrict__ rwoff,
                                                      int64_t *__restrict__ rlen, int32_t *__restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) { lwoff[n] = (int64_t)offl[n]; rwoff[n] = (int64_t)offr[n]; }
    if (t < n) {
        lwoff[t] = (int64_t)offl[t]; rwoff[t] = (int64_t)offr[t];
        llen[t] = clen[2 * t]; rlen[t] = clen[2 * t + 1];
        flags[t] = cflags[t];
    } else if (t - n < 2 * EE_CW * n) {
        const int64_t u = t - n, i = u / (2 * EE_CW);
        const int side = (int)(u % (2 * EE_CW)) / EE_CW, w = (int)(u % EE_CW);
        if (w < ((clen[2 * i + side] + 31) >> 5)) (side ? rw : lw)[(side ? offr : offl)[i] + w] = cons[u];
    }
}

// ---- order: the byte order of "Contig_<L>_<left>_<right>_<idx>" ----------------------------------------------------------------------
struct EeKey { uint64_t w0, w1, w2; int cnt; };
__device__ __forceinline__ void ee_push(EeKey &k, uint64_t nib) {
    k.w0 = (k.w0 << 4) | (k.w1 >> 60); k.w1 = (k.w1 << 4) | (k.w2 >> 60); k.w2 = (k.w2 << 4) | nib;
    k.cnt++;
}
__device__ __forceinline__ void ee_push_int(EeKey &k, int v) {       // '-' 1, '0'..'9' 2..11
    const int c = pk_int_chars(v);
    for (int q = 0; q < c; q++) {
        const char ch = pk_int_char(v, q);
        ee_push(k, ch == '-' ? 1ull : (uint64_t)(2 + ch - '0'));
    }
}
__global__ __launch_bounds__(256) void k_ee_keys(const int64_t *__restrict__ len, const int32_t *__restrict__ left, const int32_t *__restrict__ right, int64_t n,
                                                 uint64_t *__restrict__ cols /* [3][n] */) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t L = len[i];
    EeKey k{0ull, 0ull, 0ull, 0};
    ee_push_int(k, L >= 0 && L < ((int64_t)1 << 30) ? (int)L : 0);   // (a length out of range fails the call in k_ee_plan)
    ee_push(k, 12ull);                                               // '_'
    ee_push_int(k, left[i]); ee_push(k, 12ull);
    ee_push_int(k, right[i]); ee_push(k, 12ull);
    ee_push_int(k, (int)i);
    while (k.cnt < 48) ee_push(k, 0ull);                             // the end of the text sorts ahead of every character
    cols[i] = k.w0; cols[n + i] = k.w1; cols[2 * n + i] = k.w2;
}

// ---- splice (:413-562) -----------------------------------------------------------------------------------------------------------
// per position q of the order: whether the contig there is a row of the union's output (an original of 2 bases or more), whether
// 07EndExtend keeps it (2 max_k text characters or more, literals included) and the words it takes; every layout is checked here
__global__ __launch_bounds__(256) void k_ee_plan(const Fx2View in, const EeConsIn c, const uint32_t *__restrict__ perm, int min_len,
                                                 uint32_t *__restrict__ present, uint32_t *__restrict__ keep, uint32_t *__restrict__ nw, CallFlags *__restrict__ flags) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= in.n) return;
    const int64_t i = perm[q], L = in.len[i], cl = c.llen[i], cr = c.rlen[i];
    const int f = c.flags[i];
    const bool bad = L < 0 || in.woff[i + 1] - in.woff[i] != ((L + 31) >> 5) || (i == 0 && (in.woff[0] != 0 || c.lwoff[0] != 0 || c.rwoff[0] != 0)) ||
                     cl < 0 || cl > EE_LONGEST || c.lwoff[i + 1] - c.lwoff[i] != ((cl + 31) >> 5) ||
                     cr < 0 || cr > EE_LONGEST || c.rwoff[i + 1] - c.rwoff[i] != ((cr + 31) >> 5) || (f & ~3);
    const bool big = !bad && L >= ((int64_t)1 << 30);
    if (bad) atomicOr(&flags->bad, (uint32_t)EE_BAD_LAYOUT);
    if (big) atomicOr(&flags->bad, (uint32_t)EE_TOO_LONG);
    const bool there = !bad && !big && L >= 2;
    const int64_t bl = cl + L + cr, tl = bl + 3 * (f & 1) + 3 * ((f >> 1) & 1);
    const bool kept = there && tl >= min_len;
    present[q] = there ? 1u : 0u;
    keep[q] = kept ? 1u : 0u;
    nw[q] = kept ? (uint32_t)((bl + 31) >> 5) : 0u;
}
// threads [0, n): a kept contig's fields at its output position; threads [n, n + words): one output word each
__global__ __launch_bounds__(256) void k_ee_splice(const Fx2View in, const EeConsIn c, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ keep,
                                                   const uint64_t *__restrict__ nidx, const uint64_t *__restrict__ opos, const uint64_t *__restrict__ woff,
                                                   const EeSetOut o) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n = in.n;
    const int64_t words = (int64_t)woff[n];
    if (t == 0) o.woff[opos[n]] = words;
    if (t < n) {
        if (!keep[t]) return;
        const int64_t i = perm[t], at = (int64_t)opos[t];
        const int f = c.flags[i], fl = f & 1, fr = (f >> 1) & 1;
        o.woff[at] = (int64_t)woff[t];
        o.len[at] = c.llen[i] + in.len[i] + c.rlen[i];
        o.left_len[at] = (int32_t)c.llen[i] + 3 * fl; o.right_len[at] = (int32_t)c.rlen[i] + 3 * fr;
        o.flags[at] = f;
        // a flagged side's limit is 1: a field of 0 or less becomes 1, a positive one only where 1 >= the field (:440-459)
        o.left[at] = fl && in.left[i] <= 1 ? 1 : in.left[i];
        o.right[at] = fr && in.right[i] <= 1 ? 1 : in.right[i];
        o.src_idx[at] = (int32_t)i; o.new_idx[at] = (int32_t)nidx[t];
    } else if (t - n < words) {
        const int64_t w = t - n, q = pk_find(woff, n, w), i = perm[q];
        const int cl = (int)c.llen[i], L = (int)in.len[i], cr = (int)c.rlen[i];
        const int b = 32 * (int)(w - (int64_t)woff[q]);             // the word holds bases [b, b + 32) of the spliced contig
        // the left consensus REVERSED: base p of it is base cl - 1 - p of the pile, so the window is the pile's 32 bases from
        // cl - 32 - b, their order turned round
        uint64_t x = pk_rev2(pk_seg32(c.lw + c.lwoff[i], cl, cl - 32 - b));
        x |= pk_seg32(in.w + in.woff[i], L, b - cl);
        x |= pk_seg32(c.rw + c.rwoff[i], cr, b - cl - L);
        o.w[w] = pk_keep(x, cl + L + cr - b);
    }
}

// ---- text: the rows of 07EndExtend (:1268-1286) ------------------------------------------------------------------------------------
// ">Contig_<L>_<left>_<right>_<idx>_<ll>_<rl>_<new>,<sequence>\n": L the ORIGINAL contig's length, the sequence with "-1l" behind the
// reversed left consensus and "r1-" ahead of the right one where the side is flagged
struct EeRec { int f0, f1, f2, f3, f4, f5, f6, h, fl, fr, cl, tl; const uint64_t *w; };
__device__ __forceinline__ int ee_field(const EeRec &r, int k) { return k == 0 ? r.f0 : k == 1 ? r.f1 : k == 2 ? r.f2 : k == 3 ? r.f3 : k == 4 ? r.f4 : k == 5 ? r.f5 : r.f6; }
__device__ __forceinline__ EeRec ee_rec(const EeSetIn &v, int64_t i, bool ok) {
    EeRec r;
    const int f = ok ? v.flags[i] : 0;
    r.fl = f & 1; r.fr = (f >> 1) & 1;
    r.f4 = ok ? v.left_len[i] : 0; r.f5 = ok ? v.right_len[i] : 0;
    r.cl = r.f4 - 3 * r.fl;
    const int bl = ok ? (int)v.len[i] : 0;
    r.f0 = bl - r.cl - (r.f5 - 3 * r.fr);
    r.f1 = v.left[i]; r.f2 = v.right[i]; r.f3 = v.src_idx[i]; r.f6 = v.new_idx[i];
    r.tl = bl + 3 * r.fl + 3 * r.fr;
    r.h = 8;                                                        // ">Contig_"
#pragma unroll
    for (int k = 0; k < 7; k++) r.h += pk_int_chars(ee_field(r, k)) + 1;  // every field and the '_' or ',' behind it
    r.w = v.w + (ok ? v.woff[i] : 0);
    return r;
}
// byte q of a record: a character, or (0) base *t of the spliced contig with *run bases of that run left, this one included
__device__ __forceinline__ char ee_byte(const EeRec &r, int64_t q, int *t, int *run) {
    if (q < 8) return ">Contig_"[q];
    if (q < r.h) {
        int u = (int)q - 8;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const int v = ee_field(r, k), c = pk_int_chars(v);
            if (u < c) return pk_int_char(v, u);
            if (u == c) return k == 6 ? ',' : '_';
            u -= c + 1;
        }
    }
    int u = (int)(q - r.h);
    if (u >= r.tl) return '\n';
    const int lit1 = r.fl ? r.cl : -1;                              // where "-1l" begins
    const int lit2 = r.fr ? r.tl - r.f5 : -1;                       // where "r1-" begins
    if (lit1 >= 0 && u >= lit1 && u < lit1 + 3) return "-1l"[u - lit1];
    if (lit2 >= 0 && u >= lit2 && u < lit2 + 3) return "r1-"[u - lit2];
    const int stop = lit1 > u ? lit1 : lit2 > u ? lit2 : r.tl;
    *run = stop - u;
    *t = u - (lit1 >= 0 && u > lit1 ? 3 : 0) - (lit2 >= 0 && u > lit2 ? 3 : 0);
    return 0;
}
// per contig: the bytes of its row; the layout the header promises is checked here, before anything indexes with it
__global__ __launch_bounds__(256) void k_ee_text_sizes(const EeSetIn v, uint64_t *__restrict__ sz, CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n) return;
    const int64_t L = v.len[i];
    const int f = v.flags[i], ll = v.left_len[i] - 3 * (f & 1), rl = v.right_len[i] - 3 * ((f >> 1) & 1);
    const bool big = L >= ((int64_t)1 << 30);
    const bool bad = L < 0 || v.woff[i + 1] - v.woff[i] != ((L + 31) >> 5) || (i == 0 && v.woff[0] != 0) || (f & ~3) || ll < 0 || ll > EE_LONGEST ||
                     rl < 0 || rl > EE_LONGEST || (!big && ll + rl > L);
    if (bad) atomicOr(&flags->bad, (uint32_t)EE_BAD_LAYOUT);
    if (!bad && big) atomicOr(&flags->bad, (uint32_t)EE_TOO_LONG);
    const EeRec r = ee_rec(v, i, !bad && !big);
    sz[i] = (uint64_t)r.h + (uint64_t)r.tl + 1u;
}
// one thread per 16-byte chunk of the destination: chunk c holds the text's bytes [16 c - skew, 16 c - skew + 16) cut to [0, lim),
// skew = the destination address mod 16, so a whole chunk is a 16-byte-aligned store
__global__ __launch_bounds__(256) void k_ee_text_fill(const EeSetIn v, const uint64_t *__restrict__ toff, int64_t lim, int skew, int64_t chunks,
                                                      char *__restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    const int64_t start = 16 * c - skew;
    const int64_t b0 = start < 0 ? 0 : start, b1 = start + 16 < lim ? start + 16 : lim;
    const bool whole = b1 - b0 == 16;
    int64_t i = pk_find(toff, v.n, b0);
    EeRec r = ee_rec(v, i, true);
    int64_t q = b0 - (int64_t)toff[i], next = (int64_t)toff[i + 1];
    uint32_t o0 = 0u, o1 = 0u, o2 = 0u, o3 = 0u;
    int t = 0, run = 0;
    const char first = ee_byte(r, q, &t, &run);
    if (whole && first == 0 && run >= 16) {
        const Pk16 y = pk_letters16(r.w, t);                        // 16 bases out of one or two words
        o0 = y.a; o1 = y.b; o2 = y.c; o3 = y.d;
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int64_t b = b0 + j;
            if (b < b1) {
                if (b >= next) {                                  // the chunk crosses into the next record
                    i++;
                    r = ee_rec(v, i, true);
                    q = 0; next = (int64_t)toff[i + 1];
                }
                char ch = ee_byte(r, q, &t, &run);
                if (ch == 0) ch = (char)pk_letter(pk_base_of(r.w, t));
                const uint32_t x = (uint32_t)(uint8_t)ch << (8 * (j & 3));
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

// ---- the rows of 05FixingAgain, "Contig_<L>_<left>_<right>_<idx>,<contig>", into a packed contig set (the host form's input) ------------
__global__ __launch_bounds__(256) void k_ee_ctg_parse(const char *__restrict__ text, const int64_t *__restrict__ row_off, int64_t n, int64_t *__restrict__ len,
                                                      int32_t *__restrict__ left, int32_t *__restrict__ right, int64_t *__restrict__ bbeg, uint32_t *__restrict__ nw,
                                                      CallFlags *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = row_off[i];
    int64_t e = row_off[i + 1];
    while (e > b && (text[e - 1] == '\n' || text[e - 1] == '\r')) e--;
    int L = 0, lf = 0, rt = 0, idx = 0;
    int64_t p = b;
    const bool ok = ee_id(text, p, e, &L, &lf, &rt, &idx) && p < e && text[p] == ',' && (int64_t)idx == i && e - (p + 1) == (int64_t)L && L < (1 << 30);
    if (!ok) atomicOr(&flags->bad, (uint32_t)EE_BAD_ID);
    len[i] = ok ? L : 0; left[i] = lf; right[i] = rt; bbeg[i] = p + 1;
    nw[i] = ok ? (uint32_t)((L + 31) >> 5) : 0u;
}
__global__ __launch_bounds__(256) void k_ee_ctg_pack(const char *__restrict__ text, const int64_t *__restrict__ bbeg, const int64_t *__restrict__ len,
                                                     const uint64_t *__restrict__ woff, int64_t n, uint64_t *__restrict__ ow, int64_t *__restrict__ owoff,
                                                     CallFlags *__restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t words = (int64_t)woff[n];
    if (t <= n) owoff[t] = (int64_t)woff[t];
    if (t >= words) return;
    const int64_t i = pk_find(woff, n, t);
    const int b = 32 * (int)(t - (int64_t)woff[i]), m = (int)len[i] - b;
    const char *s = text + bbeg[i] + b;
    uint64_t x = 0ull;
    bool other = false;                                             // a contig is A, C, G and T, as the writer of 05FixingAgain writes it
    for (int j = 0; j < 32; j++) {
        if (j < m) {
            const char ch = s[j];
            other |= !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
            x |= pk_at(pk_code(ch), j);
        }
    }
    if (other) atomicOr(&flags->bad, (uint32_t)EE_BAD_ID);
    ow[t] = x;
}

static int ee_bad(rfx_ctx *ctx, uint32_t bad) {
    if (bad & EE_BAD_LAYOUT) { ctx->last_error = "end extension: a set whose word_off and len disagree, or lengths and flags that no consensus has"; return RFX_E_ARG; }
    if (bad & EE_TOO_LONG) { ctx->last_error = "end extension: a contig of 2^30 bases or more"; return RFX_E_LIMIT; }
    if (bad & EE_BAD_ID) { ctx->last_error = "end extension: a contig row that is not Contig_<L>_<left>_<right>_<idx>,<L bases of ACGT> with idx its position"; return RFX_E_ARG; }
    if (bad & EE_BAD_HIT) { ctx->last_error = "end extension: a hit that rfx_dev_map_ends does not write for these contigs and reads"; return RFX_E_ARG; }
    if (bad & EE_BAD_START) { ctx->last_error = "end extension: an alignment row whose start is no int"; return RFX_E_ARG; }
    if (bad & EE_BAD_CIGAR) { ctx->last_error = "end extension: an alignment row whose CIGAR is not ([0-9]+[A-Z=])+"; return RFX_E_ARG; }
    if (bad & EE_BAD_RANGE) { ctx->last_error = "end extension: an alignment row whose overhang lies outside its sequence"; return RFX_E_ARG; }
    return RFX_OK;
}

}  // namespace

// parse, group, pile-up: the consensus of every contig in the library's scratch, and the words both sets take
int rfx::ee_consensus_plan(rfx_ctx *ctx, const Fx2View &in, const char *d_text, const int64_t *d_row_off, int64_t n_rows, EeConsPlan &plan) {
    const int64_t n = in.n;
    plan.n = n; plan.lwords = 0; plan.rwords = 0;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "end extension: 2^31 contigs or more"; return RFX_E_LIMIT; }
    if (n_rows >= ((int64_t)1 << 31)) { ctx->last_error = "end extension: 2^31 rows or more"; return RFX_E_LIMIT; }
    if (n == 0) return RFX_OK;
    DevBuf rows, keys, vals, tk, tv, first, nwl, nwr, flags;
    const int64_t nr = std::max<int64_t>(n_rows, 1);
    RFX_ALLOC(rows, EeRow, nr); RFX_ALLOC(keys, uint64_t, nr); RFX_ALLOC(vals, uint32_t, nr);
    RFX_ALLOC(tk, uint64_t, nr); RFX_ALLOC(tv, uint32_t, nr); RFX_ALLOC(first, int64_t, n + 1);
    RFX_ALLOC(plan.cons, uint64_t, 2 * EE_CW * n); RFX_ALLOC(plan.clen, int32_t, 2 * n); RFX_ALLOC(plan.cflags, int32_t, n);
    RFX_ALLOC(nwl, uint32_t, n); RFX_ALLOC(nwr, uint32_t, n);
    RFX_ALLOC(plan.offl, uint64_t, n + 1); RFX_ALLOC(plan.offr, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    if (n_rows > 0) {
        RFX_LAUNCH_N(k_ee_parse, n_rows, d_text, d_row_off, n_rows, in.len, in.left, in.right, n, rows.as<EeRow>(), keys.as<uint64_t>(),
                     vals.as<uint32_t>(), flags.as<CallFlags>());
        int bits = 1;
        while (((int64_t)1 << bits) <= n) bits++;                   // (keys run to n)
        RFX_TRY(sort_pairs(ctx, keys.as<uint64_t>(), vals.as<uint32_t>(), n_rows, bits, tk.as<uint64_t>(), tv.as<uint32_t>()));
    }
    RFX_LAUNCH_N(k_ee_first, n + 1, keys.as<uint64_t>(), n_rows, n, first.as<int64_t>());
    RFX_LAUNCH(k_ee_pile, dim3((unsigned)n), dim3(64 * EE_WAVES), 0, d_text, rows.as<EeRow>(), vals.as<uint32_t>(), first.as<int64_t>(),
               plan.cons.as<uint64_t>(), plan.clen.as<int32_t>(), plan.cflags.as<int32_t>());
    RFX_LAUNCH_N(k_ee_cons_sizes, n, plan.clen.as<int32_t>(), n, nwl.as<uint32_t>(), nwr.as<uint32_t>());
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, nwl.as<uint32_t>(), nwr.as<uint32_t>(), plan.offl.as<uint64_t>(), plan.offr.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, plan.offl.as<uint64_t>() + n, plan.offr.as<uint64_t>() + n, nullptr, &f));
    RFX_TRY(ee_bad(ctx, f.bad));
    plan.lwords = (int64_t)f.total[0]; plan.rwords = (int64_t)f.total[1];
    return RFX_OK;
}
// the same plan from the hits of the end mapping and the read store: check and contributions, group, pile-up
int rfx::ee_consensus_plan_hits(rfx_ctx *ctx, const Fx2View &in, const uint64_t *d_words, const uint32_t *d_read_len, int wpr, const MpHits &hits,
                                int64_t n_hits, int seed, EeConsPlan &plan) {
    const int64_t n = in.n;
    plan.n = n; plan.lwords = 0; plan.rwords = 0;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "end extension: 2^31 contigs or more"; return RFX_E_LIMIT; }
    if (n_hits >= ((int64_t)1 << 31)) { ctx->last_error = "end extension: 2^31 rows or more"; return RFX_E_LIMIT; }
    if (n == 0) {
        if (n_hits > 0) { ctx->last_error = "end extension: a hit that rfx_dev_map_ends does not write for these contigs and reads"; return RFX_E_ARG; }
        return RFX_OK;
    }
    DevBuf rows, keys, vals, tk, tv, first, nwl, nwr, flags;
    const int64_t nr = std::max<int64_t>(n_hits, 1);
    RFX_ALLOC(rows, EhHit, nr); RFX_ALLOC(keys, uint64_t, nr); RFX_ALLOC(vals, uint32_t, nr);
    RFX_ALLOC(tk, uint64_t, nr); RFX_ALLOC(tv, uint32_t, nr); RFX_ALLOC(first, int64_t, n + 1);
    RFX_ALLOC(plan.cons, uint64_t, 2 * EE_CW * n); RFX_ALLOC(plan.clen, int32_t, 2 * n); RFX_ALLOC(plan.cflags, int32_t, n);
    RFX_ALLOC(nwl, uint32_t, n); RFX_ALLOC(nwr, uint32_t, n);
    RFX_ALLOC(plan.offl, uint64_t, n + 1); RFX_ALLOC(plan.offr, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    CallFlags f{};
    if (n_hits > 0) {
        RFX_LAUNCH_N(k_eh_rows, n_hits, in, d_read_len, wpr, hits, n_hits, seed, rows.as<EhHit>(), keys.as<uint64_t>(), vals.as<uint32_t>(),
                     flags.as<CallFlags>());
        RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));      // (a refused hit is not indexed with)
        RFX_TRY(ee_bad(ctx, f.bad));
        int bits = 1;
        while (((int64_t)1 << bits) <= n) bits++;                   // (keys run to n)
        RFX_TRY(sort_pairs(ctx, keys.as<uint64_t>(), vals.as<uint32_t>(), n_hits, bits, tk.as<uint64_t>(), tv.as<uint32_t>()));
    }
    RFX_LAUNCH_N(k_ee_first, n + 1, keys.as<uint64_t>(), n_hits, n, first.as<int64_t>());
    RFX_LAUNCH(k_eh_pile, dim3((unsigned)n), dim3(64 * EE_WAVES), 0, d_words, wpr, rows.as<EhHit>(), vals.as<uint32_t>(), first.as<int64_t>(),
               plan.cons.as<uint64_t>(), plan.clen.as<int32_t>(), plan.cflags.as<int32_t>());
    RFX_LAUNCH_N(k_ee_cons_sizes, n, plan.clen.as<int32_t>(), n, nwl.as<uint32_t>(), nwr.as<uint32_t>());
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, nwl.as<uint32_t>(), nwr.as<uint32_t>(), plan.offl.as<uint64_t>(), plan.offr.as<uint64_t>(), n));
    RFX_TRY(call_flags_read(ctx, flags, plan.offl.as<uint64_t>() + n, plan.offr.as<uint64_t>() + n, nullptr, &f));
    plan.lwords = (int64_t)f.total[0]; plan.rwords = (int64_t)f.total[1];
    return RFX_OK;
}
// both consensus sets into arrays that hold plan.n contigs (word_off: plan.n + 1) and plan.lwords / plan.rwords words
int rfx::ee_consensus_fill(rfx_ctx *ctx, const EeConsPlan &plan, const EeConsOut &o) {
    const int64_t n = plan.n;
    if (n == 0) {
        RFX_HIP(hipMemsetAsync(o.lwoff, 0, 8, ctx->stream)); RFX_HIP(hipMemsetAsync(o.rwoff, 0, 8, ctx->stream));
        return RFX_OK;
    }
    RFX_LAUNCH_N(k_ee_cons_emit, n + 2 * EE_CW * n, plan.cons.as<uint64_t>(), plan.clen.as<int32_t>(), plan.cflags.as<int32_t>(),
                 plan.offl.as<uint64_t>(), plan.offr.as<uint64_t>(), n, o.lw, o.lwoff, o.llen, o.rw, o.rwoff, o.rlen, o.flags);
    return RFX_OK;
}

// the order and what the spliced set takes
int rfx::ee_contigs_plan(rfx_ctx *ctx, const Fx2View &in, const EeConsIn &c, int max_k, EePlan &plan) {
    const int64_t n = in.n;
    plan.m = 0; plan.words = 0;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "end extension: 2^31 contigs or more"; return RFX_E_LIMIT; }
    if (n == 0) return RFX_OK;
    DevBuf cols, present, nw, flags;
    RFX_ALLOC(cols, uint64_t, 3 * n); RFX_ALLOC(plan.perm, uint32_t, n);
    RFX_ALLOC(present, uint32_t, n); RFX_ALLOC(plan.keep, uint32_t, n); RFX_ALLOC(nw, uint32_t, n);
    RFX_ALLOC(plan.nidx, uint64_t, n + 1); RFX_ALLOC(plan.opos, uint64_t, n + 1); RFX_ALLOC(plan.woff, uint64_t, n + 1);
    RFX_LAUNCH_N(k_ee_keys, n, in.len, in.left, in.right, n, cols.as<uint64_t>());
    RFX_TRY(sort_columns(ctx, cols.as<uint64_t>(), 3, n, plan.perm.as<uint32_t>()));
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_ee_plan, n, in, c, plan.perm.as<uint32_t>(), 2 * max_k, present.as<uint32_t>(), plan.keep.as<uint32_t>(),
                 nw.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan2_u32_to_u64(ctx, present.as<uint32_t>(), plan.keep.as<uint32_t>(), plan.nidx.as<uint64_t>(), plan.opos.as<uint64_t>(), n));
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, nw.as<uint32_t>(), plan.woff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, plan.opos.as<uint64_t>() + n, plan.woff.as<uint64_t>() + n, nullptr, &f));
    RFX_TRY(ee_bad(ctx, f.bad));
    plan.m = (int64_t)f.total[0]; plan.words = (int64_t)f.total[1];
    return RFX_OK;
}
// the spliced contigs, in output order, into arrays that hold plan.m contigs (word_off: plan.m + 1) and plan.words words
int rfx::ee_contigs_fill(rfx_ctx *ctx, const Fx2View &in, const EeConsIn &c, const EePlan &plan, const EeSetOut &o) {
    if (in.n == 0 || plan.m == 0) {
        RFX_HIP(hipMemsetAsync(o.woff, 0, 8, ctx->stream));
        return RFX_OK;
    }
    RFX_LAUNCH_N(k_ee_splice, in.n + plan.words, in, c, plan.perm.as<uint32_t>(), plan.keep.as<uint32_t>(), plan.nidx.as<uint64_t>(),
                 plan.opos.as<uint64_t>(), plan.woff.as<uint64_t>(),
                 o);
    return RFX_OK;
}

// 07EndExtend into d_text (filled up to cap, nothing at or past it); *total = the text's length; own: a buffer of the library's
int rfx::ee_text(rfx_ctx *ctx, const EeSetIn &s, char *d_text, int64_t cap, int64_t *total, DevBuf *own) {
    const int64_t n = s.n;
    *total = 0;
    if (n == 0) return RFX_OK;
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "end extension: 2^31 contigs or more"; return RFX_E_LIMIT; }
    const EeSetIn &v = s;
    DevBuf sz, toff, flags;
    RFX_ALLOC(sz, uint64_t, n); RFX_ALLOC(toff, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_ee_text_sizes, n, v, sz.as<uint64_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u64(ctx, sz.as<uint64_t>(), toff.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, toff.as<uint64_t>() + n, nullptr, nullptr, &f));
    RFX_TRY(ee_bad(ctx, f.bad));
    *total = (int64_t)f.total[0];
    if (own) {
        RFX_HIP(own->alloc((size_t)std::max<int64_t>(*total, 1), ctx->stream));
        d_text = own->as<char>(); cap = *total;
    }
    const int64_t lim = std::min<int64_t>(*total, cap);
    if (lim > 0) {
        const int skew = (int)((uintptr_t)d_text & 15);
        const int64_t chunks = ceil_div(lim + skew, 16);
        RFX_LAUNCH_N(k_ee_text_fill, chunks, v, toff.as<uint64_t>(), lim, skew, chunks, d_text);
    }
    return sync_checked(ctx);
}

// the rows of 05FixingAgain in HBM -> a packed contig set with left / right in the library's buffers
int rfx::ee_contigs_from_rows(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, CtgDev &c) {
    if (n >= ((int64_t)1 << 31)) { ctx->last_error = "end extension: 2^31 contigs or more"; return RFX_E_LIMIT; }
    RFX_TRY(ctg_alloc_rows(ctx, c, n));
    if (n == 0) {
        RFX_TRY(ctg_alloc_words(ctx, c, 0));
        RFX_HIP(hipMemsetAsync(c.woff.p, 0, 8, ctx->stream));
        return RFX_OK;
    }
    DevBuf bbeg, nw, off, flags;
    RFX_ALLOC(bbeg, int64_t, n); RFX_ALLOC(nw, uint32_t, n); RFX_ALLOC(off, uint64_t, n + 1);
    RFX_TRY(call_flags_init(ctx, flags));
    RFX_LAUNCH_N(k_ee_ctg_parse, n, d_text, d_row_off, n, c.len.as<int64_t>(), c.left.as<int32_t>(), c.right.as<int32_t>(), bbeg.as<int64_t>(),
                 nw.as<uint32_t>(), flags.as<CallFlags>());
    RFX_TRY(exclusive_scan_u32_to_u64(ctx, nw.as<uint32_t>(), off.as<uint64_t>(), n));
    CallFlags f{};
    RFX_TRY(call_flags_read(ctx, flags, off.as<uint64_t>() + n, nullptr, nullptr, &f));
    RFX_TRY(ee_bad(ctx, f.bad));
    RFX_TRY(ctg_alloc_words(ctx, c, (int64_t)f.total[0]));
    RFX_LAUNCH_N(k_ee_ctg_pack, std::max<int64_t>(c.words, n + 1), d_text, bbeg.as<int64_t>(), c.len.as<int64_t>(), off.as<uint64_t>(), n,
                 c.w.as<uint64_t>(), c.woff.as<int64_t>(), flags.as<CallFlags>());
    RFX_TRY(call_flags_read(ctx, flags, nullptr, nullptr, nullptr, &f));      // (the scratch above is read until here)
    return ee_bad(ctx, f.bad);
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------
bool rfx::ee_set_ok(const rfx_endext_set *s) {
    return s && fx2_contigs_ok(&s->set) && s->left && s->right && s->left_len && s->right_len && s->flags && s->src_idx && s->new_idx;
}
namespace {
bool ee_cons_ok(const rfx_endext_consensus *c) { return c && fx2_contigs_ok(&c->left) && fx2_contigs_ok(&c->right) && c->flags; }
bool ee_max_k(rfx_ctx *ctx, int max_k) {
    if (max_k >= 31 && max_k <= 124) return true;
    ctx->last_error = "end extension: max_k must be 31..124";
    return false;
}
}  // namespace

extern "C" {

// SAMString2ROW (:369-388) + DSProcessSAMandExtendContigs (:564-994) of P/ReflexivDSDynamicKmerMapping.java
int rfx_dev_endext_consensus(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, const char *d_text,
                             const int64_t *d_row_off, int64_t n_rows, rfx_endext_consensus *d_out) try {
    if (!ctx || !fx2_contigs_in_ok(d_in, d_left, d_right) || !text_rows_ok(d_text, d_row_off, n_rows) || !ee_cons_ok(d_out)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    EeConsPlan plan;
    RFX_TRY(ee_consensus_plan(ctx, fx2_view(d_in, d_left, d_right), d_text, d_row_off, n_rows, plan));
    const bool lfits = packed_out_fits(&d_out->left, plan.n, plan.lwords), rfits = packed_out_fits(&d_out->right, plan.n, plan.rwords);
    if (!lfits || !rfits) return RFX_E_CAP;
    RFX_TRY(ee_consensus_fill(ctx, plan, ee_cons_out(d_out)));
    d_out->left.n = d_out->right.n = plan.n;
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

// the same from the hits of the end mapping and the read store: what rfx_dev_endext_consensus gives on the rows rfx_dev_map_to_text
// writes of them, with no text made
int rfx_dev_endext_consensus_hits(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, const uint64_t *d_words,
                                  const uint32_t *d_read_len, int words_per_read, const rfx_map_hits *hits, rfx_endext_consensus *d_out) try {
    if (!ctx || !fx2_contigs_in_ok(d_in, d_left, d_right) || words_per_read < 1 || !hits || !hits->read || !hits->end || !hits->strand || !hits->offset ||
        !hits->v || hits->cap_n < 0 || hits->n < 0 || hits->n > hits->cap_n ||
        (hits->n > 0 && (!d_words || !d_read_len || hits->seed < 11 || hits->seed > 31)) || !ee_cons_ok(d_out))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    EeConsPlan plan;
    RFX_TRY(ee_consensus_plan_hits(ctx, fx2_view(d_in, d_left, d_right), d_words, d_read_len, words_per_read, mp_hits(hits), hits->n, hits->seed, plan));
    const bool lfits = packed_out_fits(&d_out->left, plan.n, plan.lwords), rfits = packed_out_fits(&d_out->right, plan.n, plan.rwords);
    if (!lfits || !rfits) return RFX_E_CAP;
    RFX_TRY(ee_consensus_fill(ctx, plan, ee_cons_out(d_out)));
    d_out->left.n = d_out->right.n = plan.n;
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

// the union, sort("ID") (:320-331), DSExtendContigs (:413-562), the index and filter of TagStringContigRDDID (:1268-1286)
int rfx_dev_endext_contigs(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right,
                           const rfx_endext_consensus *d_cons, int max_k, rfx_endext_set *d_out) try {
    if (!ctx || !fx2_contigs_in_ok(d_in, d_left, d_right) || !ee_cons_ok(d_cons) || d_cons->left.n != d_in->n || d_cons->right.n != d_in->n ||
        !ee_set_ok(d_out) || !ee_max_k(ctx, max_k))
        return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    const Fx2View v = fx2_view(d_in, d_left, d_right);
    EePlan plan;
    RFX_TRY(ee_contigs_plan(ctx, v, ee_cons_in(d_cons), max_k, plan));
    if (!packed_out_fits(&d_out->set, plan.m, plan.words)) return RFX_E_CAP;
    RFX_TRY(ee_contigs_fill(ctx, v, ee_cons_in(d_cons), plan, ee_set_out(d_out)));
    d_out->set.n = plan.m;
    return sync_checked(ctx);
} RFX_API_CATCH(ctx)

// zipWithIndex + TagStringContigRDDID (:1268-1286): the rows of 07EndExtend
int rfx_dev_endext_to_text(rfx_ctx *ctx, const rfx_endext_set *d_in, char *d_text, int64_t cap, int64_t *out_len) try {
    if (!ctx || !ee_set_ok(d_in) || d_in->set.n < 0 || !text_out_ok(d_text, cap, out_len)) return RFX_E_ARG;
    RFX_HIP(hipSetDevice(ctx->device));
    int64_t total = 0;
    RFX_TRY(ee_text(ctx, ee_set_in(d_in), d_text, cap, &total, nullptr));
    *out_len = total;
    return total > cap ? RFX_E_CAP : RFX_OK;
} RFX_API_CATCH(ctx)

// host form of the driver behind the aligner (:305-347): the text of 05FixingAgain and the alignment rows in, 07EndExtend out;
// everything between packed and in HBM: one upload each, consensus, splice and order, the text, one copy back
int rfx_endext_text(rfx_ctx *ctx, const char *contig_text, const int64_t *contig_off, int64_t n_contigs, const char *row_text, const int64_t *row_off,
                    int64_t n_rows, int max_k, char *out, int64_t cap, int64_t *out_len) try {
    if (!ctx || !text_rows_ok(contig_text, contig_off, n_contigs) || !text_rows_ok(row_text, row_off, n_rows) || !text_out_ok(out, cap, out_len) ||
        !ee_max_k(ctx, max_k))
        return RFX_E_ARG;
    if (n_contigs >= ((int64_t)1 << 31) || n_rows >= ((int64_t)1 << 31)) {       // (before an offset is read or a byte uploaded)
        ctx->last_error = "end extension: 2^31 rows or contigs, or more";
        return RFX_E_LIMIT;
    }
    RFX_HIP(hipSetDevice(ctx->device));
    DevBuf d_ct, d_co, d_rt, d_ro, d_rows;
    CtgDev ctg;
    EeConsDev cons;
    EeSetDev set;
    RFX_TRY(dyn_upload_text(ctx, contig_text, contig_off, n_contigs, d_ct, d_co));
    RFX_TRY(dyn_upload_text(ctx, row_text, row_off, n_rows, d_rt, d_ro));
    RFX_TRY(ee_contigs_from_rows(ctx, (const char *)d_ct.p, d_co.as<int64_t>(), n_contigs, ctg));
    EeConsPlan cp;
    RFX_TRY(ee_consensus_plan(ctx, fx2_view(ctg), (const char *)d_rt.p, d_ro.as<int64_t>(), n_rows, cp));
    RFX_TRY(ee_cons_alloc(ctx, cons, n_contigs, cp.lwords, cp.rwords));
    RFX_TRY(ee_consensus_fill(ctx, cp, ee_cons_out(cons)));
    EePlan plan;
    RFX_TRY(ee_contigs_plan(ctx, fx2_view(ctg), ee_cons_in(cons), max_k, plan));
    RFX_TRY(ee_set_alloc(ctx, set, plan.m, plan.words));
    RFX_TRY(ee_contigs_fill(ctx, fx2_view(ctg), ee_cons_in(cons), plan, ee_set_out(set)));
    int64_t total = 0;
    RFX_TRY(ee_text(ctx, ee_set_in(set), nullptr, 0, &total, &d_rows));
    return text_to_host(ctx, {{d_rows, total, out, cap, out_len}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"

